"""The unit sweep away from the GPU: id decoding, the coverage summary,
probe_device(unit_sweep=True) against a fake extension, and the burn-in flag."""
import itertools
import json
import struct

import pytest

from kata_xpu_device_plugin_amd.health import gpuprobe, placement
from kata_xpu_device_plugin_amd.health.placement import Unit, decode, format_unit, summarise
from kata_xpu_device_plugin_amd.tools import burnin


def hw(se=0, sh=0, cu=0, simd=0, wave=0, high=0):
    return high << 16 | se << 13 | sh << 12 | cu << 8 | simd << 4 | wave


def rec(xcd, se, cu, simd, wave=0, sh=0, **bad):
    r = [hw(se, sh, cu, simd, wave), xcd, 0, 0, 0, 0, 0, 0]
    for kind, n in bad.items():
        r[placement.KIND_WORD[kind]] = n
    return tuple(r)


def full_chip(skip=()):
    """8 XCDs × 4 SEs × 8 CUs, one 4-wave workgroup per CU."""
    rows = []
    for xcd in range(8):
        for se in range(4):
            for cu in range(8):
                if (xcd, se, cu) in skip:
                    continue
                rows += [rec(xcd, se, cu, simd) for simd in range(4)]
    return rows


# --- decode -------------------------------------------------------------------

@pytest.mark.parametrize("word,want", [
    (0xF, Unit(0, 0, 0, 0, 0, 15)),
    (0x3 << 4, Unit(0, 0, 0, 0, 3, 0)),
    (0xF << 8, Unit(0, 0, 0, 15, 0, 0)),
    (0x1 << 12, Unit(0, 0, 1, 0, 0, 0)),
    (0x7 << 13, Unit(0, 7, 0, 0, 0, 0)),
])
def test_decode_isolates_each_hw_id_field(word, want):
    assert decode(word, 0) == want


def test_decode_xcc_and_ignored_bits():
    assert decode(0, 0x7) == Unit(7, 0, 0, 0, 0, 0)
    assert decode(0, 0xFFFFFFF5).xcd == 5
    # bits 6..7 and everything above SE_ID (TG / VM / QUEUE / STATE / ME)
    assert decode(0xFFFF0000 | 0xC0, 0) == Unit(0, 0, 0, 0, 0, 0)
    u = decode(hw(se=5, sh=1, cu=9, simd=2, wave=7, high=0xBEEF), 0x13)
    assert u == Unit(xcd=3, se=5, sh=1, cu=9, simd=2, wave_slot=7)


def test_format_unit():
    assert format_unit(Unit(3, 1, 0, 7, 2, 5)) == "XCD 3 SE 1 CU 7 SIMD 2"
    assert format_unit(Unit(3, 1, 0, 7, -1, -1)) == "XCD 3 SE 1 CU 7"
    assert format_unit(Unit(3, 1, 1, 7, 2, 0)) == "XCD 3 SE 1 SH 1 CU 7 SIMD 2"


# --- summarise ----------------------------------------------------------------

def test_summarise_full_coverage_from_bytes_and_rows():
    rows = full_chip()
    raw = b"".join(struct.pack("<8I", *r) for r in rows)
    for records in (rows, raw):
        s = summarise(records, 256, 4)
        assert (s["cus_seen"], s["simds_seen"], s["simds_expected"]) == (256, 1024, 1024)
        assert s["xcds_seen"] == 8 and s["missing"] == 0
        assert s["partial_cus"] == [] and s["faulty_units"] == []
        assert s["layout_suspect"] is False


def test_summarise_cu_with_three_simds():
    rows = [r for r in full_chip() if r[:2] != (hw(1, 0, 2, 3), 4)]
    # keep whole workgroups: pad the short one with a second wave on SIMD 0
    i = rows.index(rec(4, 1, 2, 2)) + 1
    rows.insert(i, rec(4, 1, 2, 0, wave=1))
    s = summarise(rows, 256, 4)
    assert (s["cus_seen"], s["simds_seen"], s["missing"]) == (256, 1023, 1)
    assert len(s["partial_cus"]) == 1
    p = s["partial_cus"][0]
    assert (p["xcd"], p["cu_key"], p["simds_seen"]) == (4, hw(1, 0, 2) >> 8, [0, 1, 2])
    assert p["unit"] == "XCD 4 SE 1 CU 2"
    assert not s["layout_suspect"]


def test_summarise_cu_never_seen():
    s = summarise(full_chip(skip={(6, 3, 7)}), 256, 4)
    assert (s["cus_seen"], s["simds_seen"], s["missing"]) == (255, 1020, 4)
    assert s["partial_cus"] == []          # nothing to name: it was never seen
    assert not s["layout_suspect"]


def test_summarise_counts_merged_duplicates_once():
    first = full_chip(skip={(0, 0, 0)})
    s = summarise(first + full_chip(), 256, 4)
    assert (s["cus_seen"], s["simds_seen"], s["missing"]) == (256, 1024, 0)
    assert not s["layout_suspect"]


def test_summarise_accepts_sparse_cu_ids():
    rows = []
    for xcd in range(2):
        for cu in (0, 1, 3, 4, 6, 9, 12, 15):      # harvested: ids skip
            rows += [rec(xcd, 2, cu, simd) for simd in range(4)]
    s = summarise(rows, 16, 4)
    assert (s["cus_seen"], s["simds_seen"], s["missing"]) == (16, 64, 0)
    assert s["xcds_seen"] == 2 and not s["layout_suspect"]


def test_summarise_more_keys_than_cus_is_suspect():
    rows = full_chip() + [rec(8, 0, 0, simd) for simd in range(4)]
    s = summarise(rows, 256, 4)
    assert s["cus_seen"] == 257 and s["layout_suspect"] is True


def test_summarise_block_on_two_keys_is_suspect():
    rows = full_chip()
    rows[5] = rec(0, 0, 2, 1)       # second wave of block 1 claims another CU
    assert summarise(rows, 256, 4)["layout_suspect"] is True
    # the same records read as one-wave workgroups span nothing
    assert summarise(full_chip(), 256, 1)["layout_suspect"] is False


def test_summarise_faulty_units_sorted_and_aggregated():
    rows = full_chip()
    rows[rows.index(rec(5, 2, 3, 1))] = rec(5, 2, 3, 1, bf16=8)
    rows[rows.index(rec(1, 0, 6, 2))] = rec(1, 0, 6, 2, lds=1)
    rows += [rec(5, 2, 3, 1, wave=4, bf16=8, f32=2)]     # a merged launch
    s = summarise(rows, 256, 1)
    got = [(format_unit(f["unit"]), f["kind"], f["mismatches"], f["waves"])
           for f in s["faulty_units"]]
    assert got == [("XCD 1 SE 0 CU 6", "lds", 1, 1),
                   ("XCD 5 SE 2 CU 3 SIMD 1", "f32", 2, 1),
                   ("XCD 5 SE 2 CU 3 SIMD 1", "bf16", 16, 2)]


def test_unpack_rejects_ragged_input():
    with pytest.raises(ValueError):
        summarise(b"\0" * 33, 256, 4)
    with pytest.raises(ValueError):
        summarise([(1, 2, 3)], 256, 4)
    with pytest.raises(ValueError):
        summarise([], 256, 0)


# --- probe_device against a fake extension --------------------------------------

def sweep_result(rows, **over):
    d = dict(records=b"".join(struct.pack("<8I", *r) for r in rows),
             waves_per_block=4, blocks=256, lds_bytes_per_block=160 << 10,
             exclusive=True, sweep_ms=0.25, reps=64, launches=1,
             golden_ok={"f32": True, "bf16": True, "lds": True})
    d.update(over)
    return d


HEALTHY = {
    "device_info": dict(name="AMD Instinct MI355X", gcn_arch="gfx950:sramecc+:xnack-",
                        compute_units=256, total_mem_bytes=288 << 30,
                        free_mem_bytes=280 << 30, pci_bus_id=0x0a,
                        pci_domain_id=0, pci_device_id=0, warp_size=64),
    "hbm_bandwidth_probe": dict(gbps=5500.0, best_ms=1.0, bytes_moved=1 << 32,
                                copy_mismatches=0),
    "lds_bandwidth_probe": dict(tbps=140.0, burn_ms=1.0, mismatches=0),
    "hbm_latency_probe": dict(latency_ns=400.0, steps=500000, final_index=77,
                              expected_index=77),
    "pcie_bandwidth_probe": dict(h2d_gbps=55.0, d2h_gbps=54.0, bytes=256 << 20),
    "mfma_probe_f32": dict(max_abs_err=0.0, ok=True, slab_mismatches=0, blocks=512),
    "mfma_probe_bf16": dict(max_rel_err=0.0, ok=True, tflops=1800.0, burn_ms=1.0,
                            slab_mismatches=0, burn_mismatches=0),
    "memtest": dict(bytes=1 << 31, mismatches=0),
    "mfma_probe_lowp": dict(fp8_ok=True, mx_fp8_ok=True, mx_fp4_ok=True,
                            fp8_slab_mismatches=0, mx_fp8_slab_mismatches=0,
                            mx_fp4_slab_mismatches=0,
                            mx_fp8_tflops=4200.0, mx_fp4_tflops=8400.0,
                            mx_fp8_burn_mismatches=0, mx_fp4_burn_mismatches=0,
                            mx_fp8_burn_ms=4.0, mx_fp4_burn_ms=2.0, blocks=512),
    "unit_sweep_probe": sweep_result(full_chip()),
}

SWEEP_FIELDS = {
    "unit_sweep_ran": False, "sweep_cus_seen": -1, "sweep_simds_seen": -1,
    "sweep_simds_missing": -1, "sweep_launches": 0, "sweep_ms": 0.0,
    "sweep_exclusive": False, "faulty_units": [],
}


class FakeExt:
    def __init__(self, sick=None):
        self.sick = sick or {}
        self.calls = []

    def device_count(self):
        return 1

    def __getattr__(self, name):
        if name not in HEALTHY:
            raise AttributeError(name)

        def probe(*a, **kw):
            self.calls.append((name, a, kw))
            d = dict(HEALTHY[name])
            d.update(self.sick.get(name, {}))
            return d
        return probe


def run_probe(monkeypatch, sick=None, **kw):
    fake = FakeExt(sick)
    monkeypatch.setattr(gpuprobe, "_ext", lambda: fake)
    return gpuprobe.probe_device(0, **kw), fake


def test_flag_off_never_calls_the_sweep(monkeypatch):
    rep, fake = run_probe(monkeypatch, low_precision=True)
    assert rep.passed, rep.failures
    assert not [c for c in fake.calls if c[0].startswith("unit_sweep")]
    for f, default in SWEEP_FIELDS.items():
        got = getattr(rep, f)
        assert got == default and type(got) is type(default), (f, got)


def test_flag_on_healthy_passes_and_fills_fields(monkeypatch):
    rep, fake = run_probe(monkeypatch, unit_sweep=True)
    assert rep.passed and rep.failures == []
    names = [c[0] for c in fake.calls]
    assert names.count("unit_sweep_probe") == 1
    # after the MFMA probes, before memtest
    assert names.index("mfma_probe_bf16") < names.index("unit_sweep_probe") \
        < names.index("memtest")
    assert rep.unit_sweep_ran is True
    assert (rep.sweep_cus_seen, rep.sweep_simds_seen, rep.sweep_simds_missing) == (256, 1024, 0)
    assert (rep.sweep_launches, rep.sweep_ms, rep.sweep_exclusive) == (1, 0.25, True)
    assert rep.faulty_units == []
    assert set(SWEEP_FIELDS) <= set(rep.as_dict())
    json.dumps(rep.as_dict())


@pytest.mark.parametrize("low_precision", [False, True])
def test_low_precision_selects_the_kinds(monkeypatch, low_precision):
    rep, fake = run_probe(monkeypatch, unit_sweep=True, low_precision=low_precision)
    assert rep.passed, rep.failures
    (call,) = [c for c in fake.calls if c[0] == "unit_sweep_probe"]
    assert call[1] == (0, low_precision) and call[2] == {}


def test_low_precision_kinds_are_not_swept_off_gfx950(monkeypatch):
    other = {"device_info": {"gcn_arch": "gfx942:sramecc+:xnack-"}}
    rep, fake = run_probe(monkeypatch, other, unit_sweep=True, low_precision=True)
    (call,) = [c for c in fake.calls if c[0] == "unit_sweep_probe"]
    assert call[1] == (0, False)
    assert len(rep.failures) == 1 and "skipped" in rep.failures[0]


def test_one_poisoned_record_names_the_unit_and_kind(monkeypatch):
    rows = full_chip()
    rows[rows.index(rec(3, 1, 7, 2))] = rec(3, 1, 7, 2, bf16=64)
    rep, _ = run_probe(monkeypatch, {"unit_sweep_probe": sweep_result(rows)},
                       unit_sweep=True)
    assert not rep.passed
    assert len(rep.failures) == 1, rep.failures
    assert rep.failures[0].startswith(
        "unit sweep: bf16 tile wrong on XCD 3 SE 1 CU 7 SIMD 2 (64 wrong elements")
    assert "64 repetitions" in rep.failures[0]
    (f,) = rep.faulty_units
    assert (f["unit"], f["kind"], f["mismatches"], f["waves"]) == \
        ("XCD 3 SE 1 CU 7 SIMD 2", "bf16", 64, 1)
    assert (f["xcd"], f["se"], f["cu"], f["simd"]) == (3, 1, 7, 2)
    assert (f["hw_id"], f["xcc_id"]) == (hw(1, 0, 7, 2), 3)    # raw words kept
    json.dumps(rep.as_dict())


def test_lds_fault_names_the_cu_without_a_simd(monkeypatch):
    rows = full_chip()
    rows[rows.index(rec(0, 2, 5, 3))] = rec(0, 2, 5, 3, lds=1)
    rep, _ = run_probe(monkeypatch, {"unit_sweep_probe": sweep_result(rows)},
                       unit_sweep=True)
    assert len(rep.failures) == 1, rep.failures
    assert rep.failures[0].startswith("unit sweep: LDS wrong on XCD 0 SE 2 CU 5 (1 wrong")


def test_missing_simds_fail_the_report(monkeypatch):
    rows = full_chip(skip={(2, 0, 1), (2, 0, 2)})
    rep, _ = run_probe(monkeypatch,
                       {"unit_sweep_probe": sweep_result(rows, launches=3)},
                       unit_sweep=True)
    assert not rep.passed
    assert rep.failures == ["unit sweep: 8 of 1024 SIMDs never ran it"]
    assert (rep.sweep_simds_missing, rep.sweep_launches) == (8, 3)


def test_layout_suspect_fails_the_report(monkeypatch):
    rows = full_chip()
    rows[5] = rec(0, 0, 0, 1, wave=1)      # a workgroup on two CU keys
    rows += [rec(0, 0, 1, 1)]              # the displaced SIMD, seen elsewhere
    rep, _ = run_probe(monkeypatch, {"unit_sweep_probe": sweep_result(rows)},
                       unit_sweep=True)
    assert len(rep.failures) == 1, rep.failures
    assert rep.failures[0].startswith("unit sweep: hardware ids do not fit")


def test_untrusted_golden_tile_fails_the_report(monkeypatch):
    bad = sweep_result(full_chip(), golden_ok={"f32": True, "bf16": False, "lds": True})
    rep, _ = run_probe(monkeypatch, {"unit_sweep_probe": bad}, unit_sweep=True)
    assert len(rep.failures) == 1, rep.failures
    assert rep.failures[0].startswith("unit sweep: no trusted golden bf16 tile")


# --- burn-in CLI ----------------------------------------------------------------

@pytest.mark.parametrize("argv,want_sweep,want_lowp", [
    ([], None, None),
    (["--unit-sweep"], True, None),
    (["--unit-sweep", "--quick"], True, None),
    (["--unit-sweep", "--low-precision"], True, True),
    (["--low-precision"], None, True),
])
def test_burnin_flag(monkeypatch, capsys, argv, want_sweep, want_lowp):
    seen = {}

    def fake_probe_all(parallel=False, **kw):
        seen.update(kw)
        return [gpuprobe.ProbeReport(device=0, passed=True)]

    monkeypatch.setattr(burnin, "probe_all", fake_probe_all)
    assert burnin.main(argv + ["--json"]) == 0
    assert seen.get("unit_sweep") is want_sweep
    assert seen.get("low_precision") is want_lowp
    if "--quick" in argv:
        assert seen["burn_iters"] == 2000
    out = json.loads(capsys.readouterr().out)
    assert set(SWEEP_FIELDS) <= set(out[0])


def test_soak_summary_counts_passes_per_faulty_unit(monkeypatch, capsys):
    twice = {"unit": "XCD 3 SE 1 CU 7 SIMD 2", "kind": "bf16", "mismatches": 64, "waves": 1}
    once = {"unit": "XCD 0 SE 0 CU 1", "kind": "lds", "mismatches": 1, "waves": 1}
    passes = [[twice], [], [twice, once]]
    clock = itertools.count()
    calls = []

    def fake_probe_all(parallel=False, **kw):
        faulty = passes[len(calls)]
        calls.append(kw)
        return [gpuprobe.ProbeReport(device=0, passed=not faulty, faulty_units=faulty,
                                     failures=["x"] * len(faulty))]

    import time
    # the deadline is 3.6 "seconds" away and every look at the clock is one
    monkeypatch.setattr(time, "monotonic", lambda: next(clock))
    monkeypatch.setattr(burnin, "probe_all", fake_probe_all)
    assert burnin.main(["--unit-sweep", "--soak-minutes", "0.06"]) == 1
    assert len(calls) == 3 and all(kw["unit_sweep"] is True for kw in calls)
    out = json.loads(capsys.readouterr().out)
    assert (out["passes"], out["failing_passes"]) == (3, 2)
    assert out["faulty_units"] == [
        {"device": 0, "unit": "XCD 0 SE 0 CU 1", "kind": "lds", "failing_passes": 1},
        {"device": 0, "unit": "XCD 3 SE 1 CU 7 SIMD 2", "kind": "bf16", "failing_passes": 2},
    ]
