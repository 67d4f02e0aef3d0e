"""Pass/fail logic of probe_device() and probe_snapshot() against a fake
extension, and the reference helpers the GPU kernel tests rely on."""
import ctypes
import ctypes.util
import random
import struct

import numpy as np
import pytest

import kata_xpu_device_plugin_amd as pkg
from kata_xpu_device_plugin_amd.health import gpuprobe
from kata_xpu_device_plugin_amd.health.probe_poller import probe_snapshot

from refnum import bf16_round_bits, fmaf_exact


class FakeExt:
    """Stands in for _gpuprobe: healthy MI355X numbers unless overridden
    per probe via `sick={probe_name: {key: value}}`."""

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

    def __init__(self, sick=None, n_devices=1, raises=()):
        self.sick = sick or {}
        self.n_devices = n_devices
        self.raises = set(raises)

    def device_count(self):
        return self.n_devices

    def __getattr__(self, name):
        if name not in self.HEALTHY:
            raise AttributeError(name)

        def probe(dev=0, *a, **kw):
            if name in self.raises:
                raise RuntimeError(f"{name} failed: hipErrorUnknown")
            d = dict(self.HEALTHY[name])
            d.update(self.sick.get(name, {}))
            if name == "device_info":
                d["pci_bus_id"] += dev
            return d
        return probe


def run_probe(monkeypatch, sick=None, **kw):
    fake = FakeExt(sick)
    monkeypatch.setattr(gpuprobe, "_ext", lambda: fake)
    return gpuprobe.probe_device(0, **kw)


def test_all_healthy_passes(monkeypatch):
    rep = run_probe(monkeypatch)
    assert rep.passed and rep.failures == []
    assert rep.mfma_f32_ok and rep.mfma_bf16_ok
    for f in ("memtest_mismatches", "hbm_copy_mismatches", "hbm_chase_mismatches",
              "lds_mismatches", "mfma_f32_slab_mismatches",
              "mfma_bf16_slab_mismatches", "bf16_burn_mismatches"):
        assert getattr(rep, f) == 0, f


SICK = [
    ("hbm_bandwidth_probe", {"gbps": 3999.0}, "HBM bandwidth"),
    ("hbm_bandwidth_probe", {"copy_mismatches": 2}, "HBM copy"),
    ("hbm_latency_probe", {"latency_ns": 1501.0}, "HBM latency"),
    ("hbm_latency_probe", {"final_index": 78}, "pointer chase"),
    ("lds_bandwidth_probe", {"tbps": 79.0}, "LDS bandwidth"),
    ("lds_bandwidth_probe", {"mismatches": 1}, "LDS read"),
    ("pcie_bandwidth_probe", {"h2d_gbps": 19.0}, "PCIe H2D"),
    ("pcie_bandwidth_probe", {"d2h_gbps": 19.0}, "PCIe D2H"),
    ("mfma_probe_f32", {"ok": False, "max_abs_err": 1e-7}, "f32 MFMA mismatch"),
    ("mfma_probe_f32", {"slab_mismatches": 1}, "f32 MFMA: 1 blocks"),
    ("mfma_probe_bf16", {"ok": False, "max_rel_err": 0.5}, "bf16 MFMA mismatch"),
    ("mfma_probe_bf16", {"slab_mismatches": 3}, "bf16 MFMA: 3 blocks"),
    ("mfma_probe_bf16", {"burn_mismatches": 64}, "bf16 MFMA burn"),
    ("mfma_probe_bf16", {"tflops": 999.0}, "TFLOP/s"),
    ("memtest", {"mismatches": 1}, "memtest"),
]


@pytest.mark.parametrize("probe,override,needle", SICK,
                         ids=[f"{p}-{next(iter(o))}" for p, o, _ in SICK])
def test_single_sick_field_gives_one_failure(monkeypatch, probe, override, needle):
    rep = run_probe(monkeypatch, {probe: override})
    assert not rep.passed
    assert len(rep.failures) == 1, rep.failures
    assert needle in rep.failures[0], rep.failures


def test_non_gfx950_uses_low_floors_and_no_lds_floor(monkeypatch):
    other = {"device_info": {"gcn_arch": "gfx942:sramecc+:xnack-"},
             "hbm_bandwidth_probe": {"gbps": 150.0},
             "lds_bandwidth_probe": {"tbps": 1.0},
             "mfma_probe_bf16": {"tflops": 11.0}}
    rep = run_probe(monkeypatch, other)
    assert rep.passed, rep.failures
    other["hbm_bandwidth_probe"] = {"gbps": 99.0}
    other["mfma_probe_bf16"] = {"tflops": 9.0}
    rep = run_probe(monkeypatch, other)
    assert len(rep.failures) == 2, rep.failures
    # the mismatch counters are not arch-dependent
    other["lds_bandwidth_probe"] = {"tbps": 1.0, "mismatches": 5}
    rep = run_probe(monkeypatch, other)
    assert len(rep.failures) == 3, rep.failures


def test_explicit_floors_override(monkeypatch):
    rep = run_probe(monkeypatch, hbm_floor_gbps=6000.0, tflops_floor=2000.0)
    assert len(rep.failures) == 2, rep.failures


def snapshot_with(monkeypatch, fake):
    monkeypatch.setattr(pkg, "_gpuprobe", fake, raising=False)
    return probe_snapshot(quick_bytes=1 << 20, burn_iters=10)


def test_snapshot_healthy(monkeypatch):
    snap = snapshot_with(monkeypatch, FakeExt(n_devices=2))
    assert snap == {"0000:0a:00.0": True, "0000:0b:00.0": True}


@pytest.mark.parametrize("probe", ["mfma_probe_f32", "memtest", "mfma_probe_bf16"])
def test_snapshot_probe_exception_marks_unhealthy(monkeypatch, probe):
    snap = snapshot_with(monkeypatch, FakeExt(raises=[probe]))
    assert snap == {"0000:0a:00.0": False}


@pytest.mark.parametrize("probe,override", [
    ("mfma_probe_bf16", {"burn_mismatches": 1}),
    ("mfma_probe_bf16", {"ok": False}),
    ("mfma_probe_f32", {"ok": False}),
    ("memtest", {"mismatches": 1}),
])
def test_snapshot_sick_field_marks_unhealthy(monkeypatch, probe, override):
    snap = snapshot_with(monkeypatch, FakeExt({probe: override}))
    assert snap == {"0000:0a:00.0": False}


# --- reference helpers ------------------------------------------------------

def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _rand_f32(rng):
    return _f32(rng.gauss(0, 1) * 2.0 ** rng.randint(-20, 20))


def test_fraction_fmaf_matches_glibc():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = random.Random(1234)
    triples = []
    for n in range(20000):
        a, b, c = _rand_f32(rng), _rand_f32(rng), _rand_f32(rng)
        kind = n % 8
        if kind == 0:                      # exact cancellation
            a = _f32(2.0 ** rng.randint(-10, 10))
            c = -_f32(a * b)
        elif kind == 1:                    # near cancellation: c = -fl(a*b)
            c = -_f32(a * b)
        elif kind == 2:                    # subnormal results
            a = _f32(a * 2.0 ** -75)
            b = _f32(b * 2.0 ** -60)
            c = _f32(rng.randint(-8, 8) * 2.0 ** -149)
        elif kind == 3:                    # halfway cases
            a, b, c = _f32(2.0 ** 12), _f32(2.0 ** 12), _f32(rng.choice([1.0, -1.0, 3.0]))
        triples.append((a, b, c))
    triples += [(0.0, 1.0, -0.0), (-0.0, 1.0, -0.0), (-0.0, 1.0, 0.0),
                (2.0 ** 100, 2.0 ** 100, 1.0), (1.0, 1.0, -1.0)]
    bad = []
    for a, b, c in triples:
        want = np.float32(libm.fmaf(a, b, c))
        got = fmaf_exact(a, b, c)
        if want.view(np.uint32) != got.view(np.uint32):
            bad.append((a, b, c, float(want), float(got)))
    assert not bad, (len(bad), bad[:5])


def test_fraction_fmaf_is_not_double_rounding():
    """A triple where rounding a*b+c to f64 first and then to f32 differs
    from the single rounding — the reference must take the latter."""
    a = b = _f32(1.0 + 2.0 ** -12)
    c = _f32(2.0 ** -80)
    # exact = (1 + 2^-11) + 2^-24 + 2^-80: above the f32 tie by 2^-80 only,
    # which an f64 intermediate cannot hold
    twice = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    once = fmaf_exact(a, b, c)
    assert float(twice) == 1.0 + 2.0 ** -11
    assert float(once) == 1.0 + 2.0 ** -11 + 2.0 ** -23


def test_bf16_round_matches_torch():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(50000) * 2.0 ** rng.integers(-30, 30, 50000)).astype(np.float32)
    # exact ties (low 16 bits == 0x8000) with both parities of the kept lsb,
    # and the neighbours just above and below the tie
    base = rng.integers(0x0080, 0x7F00, 4096).astype(np.uint32) << 16
    ties = np.concatenate([base | 0x8000, base | 0x8001, base | 0x7FFF,
                           (base | 0x8000) ^ 0x80000000])
    x = np.concatenate([x, ties.view(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, 3.3895314e38],
                                 np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = bf16_round_bits(x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
