"""Pass/fail logic of probe_device(matrix_formats=True) against fake
extensions — the usual fake for _gpuprobe, which knows nothing of the new
module, and a second one for _gpuprobe_formats — and the burn-in flag."""
import json

import pytest

from kata_xpu_device_plugin_amd.health import gpuprobe
from kata_xpu_device_plugin_amd.tools import burnin

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
}

F64_RATE = gpuprobe.F64_TFLOPS_FLOOR_MI355X * 2
I8_RATE = gpuprobe.I8_TOPS_FLOOR_MI355X * 2

HEALTHY_FORMATS = {
    "mfma_probe_formats": dict(
        f64_ok=True, f16_ok=True, i8_ok=True, sparse_f16_ok=True,
        f64_slab_mismatches=0, f16_slab_mismatches=0, i8_slab_mismatches=0,
        sparse_f16_slab_mismatches=0, f64_tflops=F64_RATE, i8_tops=I8_RATE,
        f64_burn_mismatches=0, i8_burn_mismatches=0, f64_burn_ms=9.0, i8_burn_ms=3.0,
        blocks=512),
}

FORMAT_FIELDS = {
    "mfma_f64_ok": False, "mfma_f16_ok": False, "mfma_i8_ok": False,
    "mfma_sparse_f16_ok": False,
    "mfma_f64_slab_mismatches": -1, "mfma_f16_slab_mismatches": -1,
    "mfma_i8_slab_mismatches": -1, "mfma_sparse_f16_slab_mismatches": -1,
    "f64_tflops": 0.0, "i8_tops": 0.0,
    "f64_burn_mismatches": -1, "i8_burn_mismatches": -1,
}


class FakeExt:
    def __init__(self, table, sick=None):
        self.table = table
        self.sick = sick or {}
        self.calls = []

    def device_count(self):
        return 1

    def __getattr__(self, name):
        if name not in self.table:
            raise AttributeError(name)

        def probe(*a, **kw):
            self.calls.append((name, a, kw))
            d = dict(self.table[name])
            d.update(self.sick.get(name, {}))
            return d
        return probe


def run_probe(monkeypatch, sick=None, **kw):
    fake = FakeExt(HEALTHY, sick)
    formats = FakeExt(HEALTHY_FORMATS, sick)
    loads = []
    monkeypatch.setattr(gpuprobe, "_ext", lambda: fake)
    monkeypatch.setattr(gpuprobe, "_ext_formats", lambda: loads.append(1) or formats)
    rep = gpuprobe.probe_device(0, **kw)
    return rep, fake, formats, loads


BASE_CALLS = ["device_info", "hbm_bandwidth_probe", "lds_bandwidth_probe",
              "hbm_latency_probe", "pcie_bandwidth_probe", "mfma_probe_f32",
              "mfma_probe_bf16", "memtest"]


def test_floors_are_measured_constants():
    assert gpuprobe.F64_TFLOPS_FLOOR_MI355X > 0
    assert 0 < gpuprobe.I8_TOPS_FLOOR_MI355X <= 0.4 * 5000


def test_flag_off_never_loads_the_formats_extension(monkeypatch):
    rep, fake, formats, loads = run_probe(monkeypatch)
    assert rep.passed, rep.failures
    assert loads == [] and formats.calls == []
    assert [c[0] for c in fake.calls] == BASE_CALLS        # the sequence as it was
    for f, default in FORMAT_FIELDS.items():
        got = getattr(rep, f)
        assert got == default and type(got) is type(default), (f, got)


def test_flag_on_healthy_passes_and_fills_fields(monkeypatch):
    rep, fake, formats, loads = run_probe(monkeypatch, matrix_formats=True, burn_iters=1234)
    assert rep.passed and rep.failures == []
    assert loads == [1]
    assert [(c[0], c[1]) for c in formats.calls] == [("mfma_probe_formats", (0, 1234))]
    # the first extension sees exactly the calls it saw before, in order
    assert [c[0] for c in fake.calls] == BASE_CALLS
    assert rep.mfma_f64_ok and rep.mfma_f16_ok and rep.mfma_i8_ok and rep.mfma_sparse_f16_ok
    assert (rep.f64_tflops, rep.i8_tops) == (F64_RATE, I8_RATE)
    for f, default in FORMAT_FIELDS.items():
        got = getattr(rep, f)
        assert type(got) is type(default), (f, got)
        if isinstance(default, int) and not isinstance(default, bool):
            assert got == 0, f
    d = rep.as_dict()
    assert set(FORMAT_FIELDS) <= set(d)
    assert json.loads(json.dumps(d))["i8_tops"] == I8_RATE


SICK = [
    ({"f64_ok": False}, "f64 MFMA mismatch"),
    ({"f16_ok": False}, "f16 MFMA mismatch"),
    ({"i8_ok": False}, "i8 MFMA mismatch"),
    ({"sparse_f16_ok": False}, "2:4-sparse f16 MFMA mismatch"),
    ({"f64_slab_mismatches": 2}, "f64 MFMA: 2 blocks"),
    ({"f16_slab_mismatches": 3}, "f16 MFMA: 3 blocks"),
    ({"i8_slab_mismatches": 1}, "i8 MFMA: 1 blocks"),
    ({"sparse_f16_slab_mismatches": 7}, "2:4-sparse f16 MFMA: 7 blocks"),
    ({"f64_burn_mismatches": 64}, "f64 MFMA burn: 64 lanes"),
    ({"i8_burn_mismatches": 5}, "i8 MFMA burn: 5 lanes"),
    ({"f64_tflops": gpuprobe.F64_TFLOPS_FLOOR_MI355X - 1},
     f"f64 MFMA {gpuprobe.F64_TFLOPS_FLOOR_MI355X - 1:.0f} TFLOP/s < floor"),
    ({"i8_tops": gpuprobe.I8_TOPS_FLOOR_MI355X - 1},
     f"i8 MFMA {gpuprobe.I8_TOPS_FLOOR_MI355X - 1:.0f} TOP/s < floor"),
]


@pytest.mark.parametrize("override,needle", SICK, ids=[next(iter(o)) for o, _ in SICK])
def test_single_sick_field_gives_one_failure(monkeypatch, override, needle):
    rep, *_ = run_probe(monkeypatch, {"mfma_probe_formats": override}, matrix_formats=True)
    assert not rep.passed
    assert len(rep.failures) == 1, rep.failures
    assert rep.failures[0].startswith(needle), rep.failures
    # the sick value is reported in its field, the others stay healthy
    key, value = next(iter(override.items()))
    field = key if key in FORMAT_FIELDS else f"mfma_{key}"
    assert getattr(rep, field) == value


def test_rates_at_the_floor_pass(monkeypatch):
    at = {"f64_tflops": gpuprobe.F64_TFLOPS_FLOOR_MI355X,
          "i8_tops": gpuprobe.I8_TOPS_FLOOR_MI355X}
    rep, *_ = run_probe(monkeypatch, {"mfma_probe_formats": at}, matrix_formats=True)
    assert rep.passed, rep.failures


def test_explicit_floors_override(monkeypatch):
    rep, *_ = run_probe(monkeypatch, matrix_formats=True,
                        f64_tflops_floor=F64_RATE + 1, i8_tops_floor=I8_RATE + 1)
    assert len(rep.failures) == 2, rep.failures
    assert rep.failures[0].startswith("f64 MFMA") and rep.failures[1].startswith("i8 MFMA")
    slow = {"mfma_probe_formats": {"f64_tflops": 1.0, "i8_tops": 2.0}}
    rep, *_ = run_probe(monkeypatch, slow, matrix_formats=True,
                        f64_tflops_floor=0.5, i8_tops_floor=1.5)
    assert rep.passed, rep.failures
    # the floors are not consulted with the flag off
    rep, *_ = run_probe(monkeypatch, f64_tflops_floor=1e9, i8_tops_floor=1e9)
    assert rep.passed, rep.failures


def test_other_arch_skips_with_one_failure(monkeypatch):
    other = {"device_info": {"gcn_arch": "gfx942:sramecc+:xnack-"}}
    rep, fake, formats, loads = run_probe(monkeypatch, other, matrix_formats=True)
    assert loads == [] and formats.calls == []
    assert len(rep.failures) == 1, rep.failures
    assert "skipped" in rep.failures[0] and "gfx942" in rep.failures[0]
    assert rep.failures[0].startswith("matrix-format MFMA probes skipped")
    assert not rep.passed
    for f, default in FORMAT_FIELDS.items():
        assert getattr(rep, f) == default, f
    rep, *_ = run_probe(monkeypatch, other)
    assert rep.passed, rep.failures


def test_probe_all_passes_the_keyword_through(monkeypatch):
    fake, formats = FakeExt(HEALTHY), FakeExt(HEALTHY_FORMATS)
    monkeypatch.setattr(gpuprobe, "_ext", lambda: fake)
    monkeypatch.setattr(gpuprobe, "_ext_formats", lambda: formats)
    reps = gpuprobe.probe_all(matrix_formats=True, i8_tops_floor=I8_RATE + 1)
    assert len(reps) == 1 and len(reps[0].failures) == 1
    assert reps[0].mfma_sparse_f16_ok


def test_missing_formats_extension_is_an_error_not_a_pass(monkeypatch):
    """No quiet fall-back: with the flag on and the extension not importable
    the probe raises."""
    import builtins
    real_import = builtins.__import__

    def no_formats(name, globals=None, locals=None, fromlist=(), level=0):
        if fromlist and "_gpuprobe_formats" in fromlist:
            raise ImportError("not built")
        return real_import(name, globals, locals, fromlist, level)

    monkeypatch.setattr(builtins, "__import__", no_formats)
    with pytest.raises(RuntimeError, match="_gpuprobe_formats"):
        gpuprobe._ext_formats()


@pytest.mark.parametrize("argv,want", [
    ([], None),
    (["--quick"], None),
    (["--low-precision"], None),
    (["--matrix-formats"], True),
    (["--matrix-formats", "--quick", "--low-precision"], True),
])
def test_burnin_flag(monkeypatch, capsys, argv, want):
    seen = {}

    def fake_probe_all(parallel=False, **kw):
        seen.update(kw)
        return [gpuprobe.ProbeReport(device=0, passed=True)]

    monkeypatch.setattr(burnin, "probe_all", fake_probe_all)
    assert burnin.main(argv + ["--json"]) == 0
    assert seen.get("matrix_formats") is want
    if "--quick" in argv:
        assert seen["burn_iters"] == 2000
    out = json.loads(capsys.readouterr().out)
    assert set(FORMAT_FIELDS) <= set(out[0])
    assert "--matrix-formats" in burnin.__doc__
