"""GPU-tier tests: run on a real MI355X via gpurun / the driver.

These exercise the HIP gfx950 probe extension (the native compute path of
this control-plane project) and live-node discovery. Every test fails
loudly if the extension is missing — no silent CPU fallback.
"""
import os

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    from kata_xpu_device_plugin_amd import _gpuprobe
    if _gpuprobe.device_count() == 0:
        pytest.fail("no GPU visible — these tests require a MI355X")
    return _gpuprobe


def test_device_info(gp):
    info = gp.device_info(0)
    assert "gfx950" in info["gcn_arch"], info
    assert info["warp_size"] == 64
    assert info["compute_units"] >= 200  # MI355X: 256
    # 288 GB HBM3E per GPU
    assert info["total_mem_bytes"] > 250 * (1 << 30), info


def test_mfma_f32_exact(gp):
    """f32-input MFMA is exact f32 (guide: ≡ fmaf chain bitwise)."""
    r = gp.mfma_probe_f32(0)
    assert r["ok"], f"max_abs_err={r['max_abs_err']}"


def test_mfma_bf16_tile_and_burn(gp):
    r = gp.mfma_probe_bf16(0, 20000)
    assert r["ok"], f"max_rel_err={r['max_rel_err']}"
    # matrix cores must deliver real throughput (dense peak ≈2.5 PF;
    # this simple burn must clear 1 PF on healthy silicon)
    assert r["tflops"] > 1000, r


def test_hbm_bandwidth(gp):
    r = gp.hbm_bandwidth_probe(0, 1 << 31, 5)
    # ≈6.3 TB/s achievable; flag anything under 4 TB/s
    assert r["gbps"] > 4000, r


def test_memtest(gp):
    r = gp.memtest(0, 1 << 31)
    assert r["mismatches"] == 0, r


def test_probe_device_report(gp):
    from kata_xpu_device_plugin_amd.health.gpuprobe import probe_device
    rep = probe_device(0, bandwidth_bytes=256 << 20, memtest_bytes=256 << 20,
                       burn_iters=4000)
    assert rep.passed, rep.failures
    assert "gfx950" in rep.gcn_arch
    for f in ("memtest_mismatches", "hbm_copy_mismatches", "hbm_chase_mismatches",
              "lds_mismatches", "mfma_f32_slab_mismatches",
              "mfma_bf16_slab_mismatches", "bf16_burn_mismatches"):
        assert getattr(rep, f) == 0, (f, rep.as_dict())


def test_live_node_discovery():
    """On the GPU box the real sysfs has amdgpu-bound AMD functions; the
    scanner must see them (driver filter intentionally excludes them from
    scheduling — they are not vfio-bound)."""
    from kata_xpu_device_plugin_amd.config import Config
    from kata_xpu_device_plugin_amd.discovery.sysfs import scan_functions

    cfg = Config(sysfs_root="/sys", native="require")
    fns = scan_functions(cfg)
    gpus = [f for f in fns if f.is_gpu]
    assert gpus, "no AMD GPU functions in live sysfs"
    assert all(f.vendor == 0x1002 for f in fns)


def test_live_kfd_topology():
    from kata_xpu_device_plugin_amd.topology.kfd import read_kfd_topology

    nodes = [n for n in read_kfd_topology("/sys") if n.is_gpu]
    assert nodes, "KFD shows no GPUs"
    n = nodes[0]
    assert n.bdf is not None
    # gfx950 → target version 9.5.x
    assert n.gfx_target_version // 10000 == 9, n.gfx_target_version


def test_ident_tool_runs():
    from kata_xpu_device_plugin_amd.config import Config
    from kata_xpu_device_plugin_amd.tools.ident import collect

    doc = collect(Config())
    assert doc["functions"], doc


def test_pcie_bandwidth(gp):
    r = gp.pcie_bandwidth_probe(0, 256 << 20, 5)
    # Gen5 x16 spec 63 GB/s; require a sane link both directions
    assert r["h2d_gbps"] > 20, r
    assert r["d2h_gbps"] > 20, r


def test_lds_bandwidth(gp):
    """ds_read_b128 streaming: ≈150 TB/s chip-wide per the microarch
    tables; flag anything under 80 TB/s."""
    r = gp.lds_bandwidth_probe(0, 100000)
    assert r["tbps"] > 80, r


def test_hbm_latency(gp):
    """Dependent-chain HBM load latency ≈900 cycles ≈ 375-450 ns at
    2.0-2.4 GHz; flag pathological latency (>1.5 µs)."""
    r = gp.hbm_latency_probe(0, 1 << 30, 2000000)
    assert 100 < r["latency_ns"] < 1500, r


def test_probe_snapshot_bdf_mapping(gp):
    """HIP device → BDF mapping must land on a real sysfs AMD GPU function."""
    from kata_xpu_device_plugin_amd.config import Config
    from kata_xpu_device_plugin_amd.discovery.sysfs import scan_functions
    from kata_xpu_device_plugin_amd.health.probe_poller import probe_snapshot

    snap = probe_snapshot(quick_bytes=32 << 20, burn_iters=500)
    assert snap, "at least one HIP-visible GPU expected"
    assert all(snap.values()), snap
    fns = {f.bdf for f in scan_functions(Config(sysfs_root="/sys")) if f.is_gpu}
    for bdf in snap:
        assert bdf in fns, (bdf, sorted(fns))


def test_amdsmi_live_snapshot():
    """amd-smi health snapshot must return real data for the amdgpu-bound
    GPU (guards against silently-wrong amdsmi API names: every call is
    defensively wrapped, so only a live check can notice)."""
    from kata_xpu_device_plugin_amd.health.amdsmi_health import snapshot

    snap = snapshot()
    assert snap, "amd-smi saw no devices on a GPU box"
    dh = next(iter(snap.values()))
    assert dh.bdf.count(":") == 2
    assert dh.healthy
    assert dh.temperature_c is not None and 10 < dh.temperature_c < 105, (
        "temperature missing — amdsmi temp API name/enum likely wrong")


def test_amdsmi_live_xgmi_telemetry():
    """xGMI link telemetry on live silicon: the API-probing ladder in
    _read_xgmi_links must produce a well-formed (possibly empty on a
    single-GPU box with no fabric peers) link list, never crash, and any
    reported link must carry a sane index/status/error triple."""
    from kata_xpu_device_plugin_amd.health.amdsmi_health import snapshot

    snap = snapshot()
    assert snap, "amd-smi saw no devices on a GPU box"
    for dh in snap.values():
        assert isinstance(dh.xgmi_links, list)
        for link in dh.xgmi_links:
            assert link.index >= 0
            assert link.status in ("up", "down", "disabled", "unknown")
            assert link.errors >= 0
        # a healthy lone GPU must not be reported fabric-sick
        if not dh.xgmi_links:
            assert not dh.xgmi_sick


def test_partition_state_live_node():
    """Partition sysfs on live MI355X (amdgpu-bound): current compute mode
    is one of the defined modes and is in the advertised available set
    (read-only — never mutate a shared lease box)."""
    from kata_xpu_device_plugin_amd.config import Config
    from kata_xpu_device_plugin_amd.tools.partition import (
        COMPUTE_MODES, MEMORY_MODES, list_states)

    states = [s for s in list_states(Config()) if s.driver == "amdgpu"]
    assert states, "no amdgpu-bound PFs visible"
    supported = [s for s in states if s.supported]
    for st in supported:
        if st.compute_current:
            assert st.compute_current in COMPUTE_MODES, st
            if st.compute_available:
                assert st.compute_current in st.compute_available
        if st.memory_current:
            assert st.memory_current in MEMORY_MODES, st
    # informational: record what the silicon exposes
    print("partition states:", [
        (s.bdf, s.compute_current, s.compute_available,
         s.memory_current, s.memory_available) for s in states])


def test_doctor_live_node():
    """kxdp-doctor on the live box: amdgpu-bound GPUs → pre-provisioning
    verdict (exit 0) with real discovery/topology/amd-smi content."""
    from kata_xpu_device_plugin_amd.config import Config
    from kata_xpu_device_plugin_amd.tools.doctor import diagnose

    doc = diagnose(Config())
    assert not doc["problems"], doc["problems"]
    assert doc["discovery"]["functions"] >= 1
    assert any(g["driver"] == "amdgpu" for g in doc["gpus"])
    assert doc["amdsmi"], "amd-smi must see the amdgpu-bound GPU"
