"""GPU-tier tests of what the timed probes return, at the smallest sizes that
still take each one through its warm-up and its timed launch: the key set,
finite positive times and rates, and clean self-checks. No rate floors: toy
sizes measure launch overhead."""
import math

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    from kata_xpu_device_plugin_amd import _gpuprobe
    if _gpuprobe.device_count() == 0:
        pytest.fail("no GPU visible — these tests require a MI355X")
    return _gpuprobe


def check(result, keys, positive):
    """Key set, finite positive measurements, and every self-check clean."""
    assert set(result) == keys
    for k in positive:
        assert math.isfinite(result[k]) and result[k] > 0, (k, result[k])
    for k, v in result.items():
        if k.endswith("mismatches"):
            assert v == 0, (k, v)
        if k == "ok" or k.endswith("_ok"):
            assert v is True, (k, v)


def test_hbm_bandwidth_probe(gp):
    r = gp.hbm_bandwidth_probe(0, 1 << 20, 2)
    check(r, {"gbps", "best_ms", "bytes_moved", "copy_mismatches"}, ["gbps", "best_ms"])


def test_lds_bandwidth_probe(gp):
    r = gp.lds_bandwidth_probe(0, 256)
    check(r, {"tbps", "burn_ms", "mismatches"}, ["tbps", "burn_ms"])


def test_hbm_latency_probe(gp):
    r = gp.hbm_latency_probe(0, 1 << 16, 1000)
    check(r, {"latency_ns", "steps", "final_index", "expected_index"}, ["latency_ns"])
    assert r["final_index"] == r["expected_index"]


def test_pcie_bandwidth_probe(gp):
    r = gp.pcie_bandwidth_probe(0, 1 << 20, 2)
    check(r, {"h2d_gbps", "d2h_gbps", "bytes"}, ["h2d_gbps", "d2h_gbps"])


def test_mfma_probe_bf16(gp):
    r = gp.mfma_probe_bf16(0, 64)
    check(r, {"max_rel_err", "slab_mismatches", "burn_mismatches", "ok", "tflops",
              "burn_ms"}, ["tflops", "burn_ms"])


def test_mfma_probe_lowp(gp):
    r = gp.mfma_probe_lowp(0, 64)
    check(r, {"fp8_ok", "mx_fp8_ok", "mx_fp4_ok", "fp8_slab_mismatches",
              "mx_fp8_slab_mismatches", "mx_fp4_slab_mismatches", "mx_fp8_tflops",
              "mx_fp4_tflops", "mx_fp8_burn_mismatches", "mx_fp4_burn_mismatches",
              "mx_fp8_burn_ms", "mx_fp4_burn_ms", "blocks"},
          ["mx_fp8_tflops", "mx_fp4_tflops", "mx_fp8_burn_ms", "mx_fp4_burn_ms"])
