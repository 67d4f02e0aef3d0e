"""Pass/fail logic of probe_device(low_precision=True) against a fake
extension that also provides mfma_probe_lowp, and the burn-in flag."""
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
    "mfma_probe_lowp": dict(fp8_ok=True, mx_fp8_ok=True, mx_fp4_ok=True,
                            fp8_slab_mismatches=0, mx_fp8_slab_mismatches=0,
                            mx_fp4_slab_mismatches=0,
                            mx_fp8_tflops=4200.0, mx_fp4_tflops=8400.0,
                            mx_fp8_burn_mismatches=0, mx_fp4_burn_mismatches=0,
                            mx_fp8_burn_ms=4.0, mx_fp4_burn_ms=2.0, blocks=512),
}

LOWP_FIELDS = {
    "mfma_fp8_ok": False, "mfma_mx_fp8_ok": False, "mfma_mx_fp4_ok": False,
    "mx_fp8_tflops": 0.0, "mx_fp4_tflops": 0.0,
    "mfma_fp8_slab_mismatches": -1, "mfma_mx_fp8_slab_mismatches": -1,
    "mfma_mx_fp4_slab_mismatches": -1,
    "mx_fp8_burn_mismatches": -1, "mx_fp4_burn_mismatches": -1,
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


def test_flag_off_never_calls_the_new_entry_point(monkeypatch):
    rep, fake = run_probe(monkeypatch)
    assert rep.passed, rep.failures
    assert "mfma_probe_lowp" not in [c[0] for c in fake.calls]
    for f, default in LOWP_FIELDS.items():
        got = getattr(rep, f)
        assert got == default and type(got) is type(default), (f, got)


def test_flag_on_healthy_passes_and_fills_fields(monkeypatch):
    rep, fake = run_probe(monkeypatch, low_precision=True, burn_iters=1234)
    assert rep.passed and rep.failures == []
    assert [c[1] for c in fake.calls if c[0] == "mfma_probe_lowp"] == [(0, 1234)]
    assert rep.mfma_fp8_ok and rep.mfma_mx_fp8_ok and rep.mfma_mx_fp4_ok
    assert (rep.mx_fp8_tflops, rep.mx_fp4_tflops) == (4200.0, 8400.0)
    for f, default in LOWP_FIELDS.items():
        if isinstance(default, int) and not isinstance(default, bool):
            assert getattr(rep, f) == 0, f
    assert set(LOWP_FIELDS) <= set(rep.as_dict())


SICK = [
    ({"fp8_ok": False}, "fp8 MFMA mismatch"),
    ({"mx_fp8_ok": False}, "MX-fp8 MFMA mismatch"),
    ({"mx_fp4_ok": False}, "MX-fp4 MFMA mismatch"),
    ({"fp8_slab_mismatches": 2}, "fp8 MFMA: 2 blocks"),
    ({"mx_fp8_slab_mismatches": 3}, "MX-fp8 MFMA: 3 blocks"),
    ({"mx_fp4_slab_mismatches": 1}, "MX-fp4 MFMA: 1 blocks"),
    ({"mx_fp8_burn_mismatches": 64}, "MX-fp8 MFMA burn"),
    ({"mx_fp4_burn_mismatches": 5}, "MX-fp4 MFMA burn"),
    ({"mx_fp8_tflops": gpuprobe.MX_FP8_TFLOPS_FLOOR_MI355X - 1},
     f"MX-fp8 MFMA {gpuprobe.MX_FP8_TFLOPS_FLOOR_MI355X - 1:.0f} TFLOP/s < floor"),
    ({"mx_fp4_tflops": gpuprobe.MX_FP4_TFLOPS_FLOOR_MI355X - 1},
     f"MX-fp4 MFMA {gpuprobe.MX_FP4_TFLOPS_FLOOR_MI355X - 1:.0f} TFLOP/s < floor"),
]


@pytest.mark.parametrize("override,needle", SICK, ids=[next(iter(o)) for o, _ in SICK])
def test_single_sick_field_gives_one_failure(monkeypatch, override, needle):
    rep, _ = run_probe(monkeypatch, {"mfma_probe_lowp": override}, low_precision=True)
    assert not rep.passed
    assert len(rep.failures) == 1, rep.failures
    assert rep.failures[0].startswith(needle), rep.failures


def test_rates_at_the_floor_pass(monkeypatch):
    at = {"mx_fp8_tflops": gpuprobe.MX_FP8_TFLOPS_FLOOR_MI355X,
          "mx_fp4_tflops": gpuprobe.MX_FP4_TFLOPS_FLOOR_MI355X}
    rep, _ = run_probe(monkeypatch, {"mfma_probe_lowp": at}, low_precision=True)
    assert rep.passed, rep.failures


def test_explicit_floors_override(monkeypatch):
    rep, _ = run_probe(monkeypatch, low_precision=True,
                       fp8_tflops_floor=4201.0, fp4_tflops_floor=8401.0)
    assert len(rep.failures) == 2, rep.failures
    assert "4201" in rep.failures[0] and "8401" in rep.failures[1]
    slow = {"mfma_probe_lowp": {"mx_fp8_tflops": 10.0, "mx_fp4_tflops": 20.0}}
    rep, _ = run_probe(monkeypatch, slow, low_precision=True,
                       fp8_tflops_floor=5.0, fp4_tflops_floor=15.0)
    assert rep.passed, rep.failures
    # the floors are not consulted with the flag off
    rep, _ = run_probe(monkeypatch, fp8_tflops_floor=1e9, fp4_tflops_floor=1e9)
    assert rep.passed, rep.failures


def test_other_arch_skips_with_one_failure(monkeypatch):
    other = {"device_info": {"gcn_arch": "gfx942:sramecc+:xnack-"}}
    rep, fake = run_probe(monkeypatch, other, low_precision=True)
    assert "mfma_probe_lowp" not in [c[0] for c in fake.calls]
    assert len(rep.failures) == 1, rep.failures
    assert "skipped" in rep.failures[0] and "gfx942" in rep.failures[0]
    assert not rep.passed
    for f, default in LOWP_FIELDS.items():
        assert getattr(rep, f) == default, f
    # and without the flag that arch is as before
    rep, _ = run_probe(monkeypatch, other)
    assert rep.passed, rep.failures


def test_probe_all_passes_the_keyword_through(monkeypatch):
    fake = FakeExt()
    monkeypatch.setattr(gpuprobe, "_ext", lambda: fake)
    reps = gpuprobe.probe_all(low_precision=True, fp4_tflops_floor=9000.0)
    assert len(reps) == 1 and len(reps[0].failures) == 1
    assert reps[0].mfma_mx_fp4_ok


@pytest.mark.parametrize("argv,want", [
    ([], None),
    (["--quick"], None),
    (["--low-precision"], True),
    (["--low-precision", "--quick"], True),
])
def test_burnin_flag(monkeypatch, capsys, argv, want):
    seen = {}

    def fake_probe_all(parallel=False, **kw):
        seen.update(kw)
        rep = gpuprobe.ProbeReport(device=0, passed=True)
        return [rep]

    monkeypatch.setattr(burnin, "probe_all", fake_probe_all)
    assert burnin.main(argv + ["--json"]) == 0
    assert seen.get("low_precision") is want
    if "--quick" in argv:
        assert seen["burn_iters"] == 2000
    out = json.loads(capsys.readouterr().out)
    assert set(LOWP_FIELDS) <= set(out[0])
