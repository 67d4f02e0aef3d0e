"""_gpuprobe argument validation: every bad argument is a ValueError raised
before the first HIP call, so these run on a machine without a GPU."""
import numpy as np
import pytest

gp = pytest.importorskip("kata_xpu_device_plugin_amd._gpuprobe")

A32 = np.zeros((16, 4), np.float32)
B32 = np.zeros((4, 16), np.float32)
C32 = np.zeros((16, 16), np.float32)
A16 = np.zeros((32, 16), np.uint16)
B16 = np.zeros((16, 32), np.uint16)


@pytest.mark.parametrize("call", [
    lambda: gp.device_info(-1),
    lambda: gp.hbm_bandwidth_probe(-1, 1 << 20, 1),
    lambda: gp.hbm_copy_check(-1, 1 << 20),
    lambda: gp.memtest(-1, 1 << 20),
    lambda: gp.pcie_bandwidth_probe(-1, 1 << 20, 1),
    lambda: gp.lds_bandwidth_probe(-1, 100),
    lambda: gp.lds_read_burn_run(-1, 1),
    lambda: gp.hbm_latency_probe(-1, 4096, 10),
    lambda: gp.mfma_probe_f32(-1),
    lambda: gp.mfma_probe_bf16(-1, 10),
    lambda: gp.mfma_bf16_burn_run(-1, 1),
    lambda: gp.mfma_f32_tile_run(-1, A32, B32),
    lambda: gp.mfma_bf16_tile_run(-1, A16, B16),
])
def test_negative_device(call):
    with pytest.raises(ValueError, match="dev"):
        call()


@pytest.mark.parametrize("n", [0, -1])
def test_non_positive_counts(n):
    for call in (
        lambda: gp.hbm_bandwidth_probe(0, 1 << 20, n),
        lambda: gp.pcie_bandwidth_probe(0, 1 << 20, n),
        lambda: gp.lds_bandwidth_probe(0, n),
        lambda: gp.lds_read_burn_run(0, n),
        lambda: gp.mfma_bf16_burn_run(0, n),
        lambda: gp.mfma_probe_bf16(0, n),
        lambda: gp.hbm_latency_probe(0, 4096, n),
    ):
        with pytest.raises(ValueError):
            call()


def test_bytes_below_one_element():
    with pytest.raises(ValueError):
        gp.hbm_bandwidth_probe(0, 15, 1)
    with pytest.raises(ValueError):
        gp.hbm_copy_check(0, 15)
    with pytest.raises(ValueError):
        gp.memtest(0, 7)
    with pytest.raises(ValueError):
        gp.pcie_bandwidth_probe(0, 0, 1)


@pytest.mark.parametrize("nbytes", [0, 4, 7, (1 << 34) + 4, 1 << 40])
def test_latency_probe_byte_range(nbytes):
    """Below 8 bytes the Sattolo loop's n-1 would wrap; above 2^32 elements
    the uint32 indices would."""
    with pytest.raises(ValueError):
        gp.hbm_latency_probe(0, nbytes, 10)


def test_memtest_corrupt_offset_outside_buffer():
    for offs in ([8], [0, 1 << 40], [7, 8]):
        with pytest.raises(ValueError, match="outside"):
            gp.memtest(0, 64, corrupt_offsets=offs)


@pytest.mark.parametrize("blocks", [0, -1, 1 << 20])
def test_tile_blocks_range(blocks):
    with pytest.raises(ValueError):
        gp.mfma_f32_tile_run(0, A32, B32, blocks=blocks)
    with pytest.raises(ValueError):
        gp.mfma_bf16_tile_run(0, A16, B16, blocks=blocks)


def test_burn_blocks_range():
    for blocks in (-1, 1 << 20):
        with pytest.raises(ValueError):
            gp.mfma_bf16_burn_run(0, 1, blocks)
        with pytest.raises(ValueError):
            gp.lds_read_burn_run(0, 1, blocks)


def test_f32_tile_buffers():
    bad_a = [np.zeros(63, np.float32), np.zeros((16, 4), np.float64),
             np.zeros((16, 4), np.float16), np.zeros((16, 8), np.float32)[:, ::2]]
    for a in bad_a:
        with pytest.raises(ValueError, match="A must"):
            gp.mfma_f32_tile_run(0, a, B32)
    with pytest.raises(ValueError, match="B must"):
        gp.mfma_f32_tile_run(0, A32, np.zeros(65, np.float32))
    for c in (np.zeros(64, np.float32), np.zeros((16, 16), np.float64)):
        with pytest.raises(ValueError, match="C must"):
            gp.mfma_f32_tile_run(0, A32, B32, c)


def test_bf16_tile_buffers():
    for a in (np.zeros(511, np.uint16), np.zeros((32, 16), np.float32),
              np.zeros((32, 16), np.uint8)):
        with pytest.raises(ValueError, match="A_bits must"):
            gp.mfma_bf16_tile_run(0, a, B16)
    with pytest.raises(ValueError, match="B_bits must"):
        gp.mfma_bf16_tile_run(0, A16, np.zeros((16, 16), np.uint16))
