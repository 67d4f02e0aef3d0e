"""GPU-tier tests of the placement-recording unit sweep: record shape, clean
silicon, coverage of every SIMD, attribution of a poisoned unit by hardware
id, and real repetitions. Each test is one to three launches of one workgroup
per CU; the healthy run and the coverage run are shared.
"""

import pytest

from kata_xpu_device_plugin_amd.health import placement
from kata_xpu_device_plugin_amd.health.gpuprobe import probe_device

pytestmark = pytest.mark.gpu

ALL = list(placement.KINDS)
FLIP = 1 << 22      # a mantissa bit: the poisoned element stays finite


@pytest.fixture(scope="module")
def gp():
    from kata_xpu_device_plugin_amd import _gpuprobe
    if _gpuprobe.device_count() == 0:
        pytest.fail("no GPU visible — these tests require a MI355X")
    return _gpuprobe


@pytest.fixture(scope="module")
def cus(gp):
    return gp.device_info(0)["compute_units"]


@pytest.fixture(scope="module")
def healthy(gp):
    return gp.unit_sweep_run(0, ALL, 8)


@pytest.fixture(scope="module")
def covered(gp):
    return gp.unit_sweep_probe(0, low_precision=True)


def rows_of(result):
    return placement.unpack(result["records"])


def test_records_are_well_formed(healthy):
    rows = rows_of(healthy)
    wpb = healthy["waves_per_block"]
    assert len(healthy["records"]) == healthy["blocks"] * wpb * 8 * 4
    assert len(rows) == healthy["blocks"] * wpb
    for r in rows:
        assert 0 <= (r[1] & 0xF) <= 7, hex(r[1])
    for b in range(healthy["blocks"]):
        keys = {placement.cu_key(r[0], r[1]) for r in rows[b * wpb:(b + 1) * wpb]}
        assert len(keys) == 1, (b, keys)
    assert set(healthy["golden_ok"]) == set(ALL)
    assert all(healthy["golden_ok"].values()), healthy["golden_ok"]
    assert healthy["lds_bytes_per_block"] % 4096 == 0
    assert healthy["exclusive"] == (healthy["lds_bytes_per_block"] > 80 << 10)
    assert healthy["sweep_ms"] > 0


def test_healthy_silicon_is_clean(healthy):
    dirty = [r for r in rows_of(healthy) if any(r[2:])]
    assert dirty == []


def test_coverage_of_every_simd(gp, covered, cus):
    s = placement.summarise(covered["records"], cus, covered["waves_per_block"])
    print("launches", covered["launches"], "sweep_ms", covered["sweep_ms"],
          "reps", covered["reps"], {k: s[k] for k in
                                    ("cus_seen", "simds_seen", "xcds_seen", "missing")})
    assert covered["reps"] == gp.UNIT_SWEEP_DEFAULT_REPS
    assert s["cus_seen"] == cus
    assert s["simds_seen"] == 4 * cus
    assert s["xcds_seen"] == 8
    assert s["layout_suspect"] is False
    assert covered["launches"] <= 3
    assert s["faulty_units"] == []
    assert all(covered["golden_ok"].values())


def pick_unit(covered):
    """A (xcd, cu_key, simd) that the coverage run saw, away from record 0."""
    rows = rows_of(covered)
    r = rows[len(rows) // 3]
    xcd, key = placement.cu_key(r[0], r[1])
    return xcd, key, placement.decode(r[0], r[1]).simd


@pytest.mark.parametrize("kind", ["f32", "bf16", "fp8", "mx_fp8", "mx_fp4"])
def test_poisoned_matrix_unit_is_named(gp, covered, cus, kind):
    xcd, key, simd = pick_unit(covered)
    res = gp.unit_sweep_run(0, ALL, 8, poison=(xcd, key, simd, kind, FLIP))
    word = placement.KIND_WORD[kind]
    hit = 0
    for r in rows_of(res):
        here = placement.cu_key(r[0], r[1]) == (xcd, key) and \
            placement.decode(r[0], r[1]).simd == simd
        if here:
            hit += 1
            assert r[word] == 8, r
            assert [c for i, c in enumerate(r[2:], 2) if i != word] == [0] * 5, r
        else:
            assert not any(r[2:]), r
    assert hit >= 1
    s = placement.summarise(res["records"], cus, res["waves_per_block"])
    (f,) = s["faulty_units"]
    assert f["kind"] == kind and f["mismatches"] == 8 * hit and f["waves"] == hit
    u = f["unit"]
    assert (u.xcd, u.se << 5 | u.sh << 4 | u.cu, u.simd) == (xcd, key, simd)


def test_poisoned_lds_word_is_charged_to_its_cu(gp, covered, cus):
    xcd, key, _ = pick_unit(covered)
    res = gp.unit_sweep_run(0, ALL, 8, poison=(xcd, key, 0, "lds", 0x00010000))
    on_cu = other = 0
    for r in rows_of(res):
        assert not any(r[2:7]), r
        if placement.cu_key(r[0], r[1]) == (xcd, key):
            on_cu += r[7]
        else:
            other += r[7]
    assert (on_cu, other) == (1, 0)
    (f,) = placement.summarise(res["records"], cus, res["waves_per_block"])["faulty_units"]
    assert f["kind"] == "lds" and f["unit"].simd == -1 and f["mismatches"] == 1


def test_repetitions_are_real(gp, covered, healthy):
    xcd, key, simd = pick_unit(covered)
    for reps in (1, 8):
        res = gp.unit_sweep_run(0, ["f32", "bf16"], reps,
                                poison=(xcd, key, simd, "f32", FLIP))
        bad = [r[2] for r in rows_of(res) if r[2]]
        assert bad and set(bad) == {reps}, (reps, bad)
    long_run = gp.unit_sweep_run(0, ALL, 4096)
    print("sweep_ms reps=8", healthy["sweep_ms"], "reps=4096", long_run["sweep_ms"])
    assert long_run["sweep_ms"] > healthy["sweep_ms"]
    assert not any(any(r[2:]) for r in rows_of(long_run))


def test_probe_device_with_and_without_the_sweep():
    kw = dict(bandwidth_bytes=64 << 20, memtest_bytes=64 << 20, burn_iters=2000,
              low_precision=True)
    rep = probe_device(0, unit_sweep=True, **kw)
    assert rep.passed, rep.failures
    assert rep.unit_sweep_ran is True
    assert rep.faulty_units == []
    assert rep.sweep_simds_missing == 0
    assert rep.sweep_simds_seen == 4 * rep.compute_units
    assert 1 <= rep.sweep_launches <= 3 and rep.sweep_ms > 0
    rep = probe_device(0, **kw)
    assert rep.unit_sweep_ran is False and rep.sweep_launches == 0
