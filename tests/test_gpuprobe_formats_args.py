"""Argument validation of _gpuprobe_formats: every bad argument is a
ValueError raised before the first HIP call, so these run on a machine
without a GPU."""
import numpy as np
import pytest

from kata_xpu_device_plugin_amd import _gpuprobe_formats as gf

A64, B64, C64 = np.zeros((16, 4)), np.zeros((4, 16)), np.zeros((16, 16))
A16, B16 = np.zeros((32, 16), np.uint16), np.zeros((16, 32), np.uint16)
A8, B8 = np.zeros((16, 64), np.int8), np.zeros((64, 16), np.int8)
C32 = np.zeros((16, 16), np.int32)
AS, IS, BS = (np.zeros((16, 32), np.uint16), np.zeros((16, 32), np.uint8),
              np.zeros((64, 16), np.uint16))


def f64(dev=0, A=A64, B=B64, C=None, **kw):
    return gf.mfma_f64_tile_run(dev, A, B, C, **kw)


def f16(dev=0, A=A16, B=B16, **kw):
    return gf.mfma_f16_tile_run(dev, A, B, **kw)


def i8(dev=0, A=A8, B=B8, C=None, **kw):
    return gf.mfma_i8_tile_run(dev, A, B, C, **kw)


def sp(dev=0, A=AS, idx=IS, B=BS, **kw):
    return gf.smfmac_f16_tile_run(dev, A, idx, B, **kw)


TILES = [f64, f16, i8, sp]
BURNS = [gf.mfma_f64_burn_run, gf.mfma_i8_burn_run]


@pytest.mark.parametrize("call", [
    lambda: f64(dev=-1), lambda: f16(dev=-1), lambda: i8(dev=-1), lambda: sp(dev=-1),
    lambda: gf.mfma_f64_burn_run(-1), lambda: gf.mfma_i8_burn_run(-1),
    lambda: gf.mfma_probe_formats(-1, 10),
])
def test_negative_device(call):
    with pytest.raises(ValueError, match="dev"):
        call()


@pytest.mark.parametrize("n", [0, -1])
def test_non_positive_iters(n):
    for burn in BURNS:
        with pytest.raises(ValueError, match="iters"):
            burn(0, n)
    with pytest.raises(ValueError, match="iters"):
        gf.mfma_probe_formats(0, n)


@pytest.mark.parametrize("blocks", [0, -1, 4097, 1 << 20])
def test_tile_blocks_range(blocks):
    for tile in TILES:
        with pytest.raises(ValueError, match="blocks"):
            tile(blocks=blocks)


@pytest.mark.parametrize("blocks", [-1, 65537, 1 << 20])
def test_burn_blocks_range(blocks):
    for burn in BURNS:
        with pytest.raises(ValueError, match="blocks"):
            burn(0, 1, blocks)


def bad_buffers(shape, dtype):
    """Wrong size, wrong dtype (same and other item size), wrong strides."""
    n = shape[0] * shape[1]
    other = {np.float64: [np.int64, np.uint64, np.float32],
             np.uint16: [np.int16, np.float16, np.uint8],
             np.int8: [np.uint8, np.bool_, np.int16],
             np.int32: [np.uint32, np.float32, np.int64],
             np.uint8: [np.int8, np.bool_, np.uint16]}[dtype]
    return ([np.zeros(n - 1, dtype), np.zeros(n + 1, dtype)] +
            [np.zeros(shape, t) for t in other] +
            [np.zeros((shape[0], 2 * shape[1]), dtype)[:, ::2],
             np.zeros((shape[1], shape[0]), dtype).T])


def test_f64_tile_buffers():
    for a in bad_buffers((16, 4), np.float64):
        with pytest.raises(ValueError, match="A must"):
            f64(A=a)
    for b in bad_buffers((4, 16), np.float64):
        with pytest.raises(ValueError, match="B must"):
            f64(B=b)
    for c in bad_buffers((16, 16), np.float64) + [3.0, "x"]:
        with pytest.raises(ValueError, match="C must"):
            f64(C=c)


def test_f16_tile_buffers():
    for a in bad_buffers((32, 16), np.uint16):
        with pytest.raises(ValueError, match="A_bits must"):
            f16(A=a)
    for b in bad_buffers((16, 32), np.uint16):
        with pytest.raises(ValueError, match="B_bits must"):
            f16(B=b)


def test_i8_tile_buffers():
    for a in bad_buffers((16, 64), np.int8):
        with pytest.raises(ValueError, match="A must"):
            i8(A=a)
    for b in bad_buffers((64, 16), np.int8):
        with pytest.raises(ValueError, match="B must"):
            i8(B=b)
    for c in bad_buffers((16, 16), np.int32) + [3, "x"]:
        with pytest.raises(ValueError, match="C must"):
            i8(C=c)


def test_sparse_tile_buffers():
    for a in bad_buffers((16, 32), np.uint16):
        with pytest.raises(ValueError, match="A_bits must"):
            sp(A=a)
    for i in bad_buffers((16, 32), np.uint8):
        with pytest.raises(ValueError, match="A_idx must"):
            sp(idx=i)
    for b in bad_buffers((64, 16), np.uint16):
        with pytest.raises(ValueError, match="B_bits must"):
            sp(B=b)
    with pytest.raises(ValueError, match="B_bits must"):
        sp(B=AS)                               # the kept half's shape, not dense K


@pytest.mark.parametrize("value", [4, 5, 128, 255])
@pytest.mark.parametrize("where", [0, 257, 511])
def test_sparse_index_out_of_range(value, where):
    idx = np.full((16, 32), 3, np.uint8)
    idx.reshape(-1)[where] = value
    with pytest.raises(ValueError, match="A_idx.*0..3"):
        sp(idx=idx)
