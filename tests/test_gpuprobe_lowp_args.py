"""Argument validation of the FP8 / MX entry points of _gpuprobe: every bad
argument is a ValueError raised before the first HIP call, so these run on a
machine without a GPU."""
import numpy as np
import pytest

gp = pytest.importorskip("kata_xpu_device_plugin_amd._gpuprobe")

A8 = np.zeros((16, 32), np.uint8)
B8 = np.zeros((32, 16), np.uint8)
AMX = np.zeros((16, 128), np.uint8)
BMX = np.zeros((128, 16), np.uint8)
SA = np.full((16, 4), 127, np.uint8)
SB = np.full((4, 16), 127, np.uint8)


def fp8(dev=0, A=A8, B=B8, af="e4m3", bf="e4m3", **kw):
    return gp.mfma_fp8_tile_run(dev, A, B, af, bf, **kw)


def mx(dev=0, A=AMX, B=BMX, sa=SA, sb=SB, af="e4m3", bf="e4m3", **kw):
    return gp.mfma_mx_tile_run(dev, A, B, sa, sb, af, bf, **kw)


@pytest.mark.parametrize("call", [
    lambda: fp8(dev=-1),
    lambda: mx(dev=-1),
    lambda: gp.mfma_mx_burn_run(-1, "e4m3"),
    lambda: gp.mfma_probe_lowp(-1, 10),
])
def test_negative_device(call):
    with pytest.raises(ValueError, match="dev"):
        call()


@pytest.mark.parametrize("n", [0, -1])
def test_non_positive_iters(n):
    with pytest.raises(ValueError, match="iters"):
        gp.mfma_mx_burn_run(0, "e4m3", n)
    with pytest.raises(ValueError, match="iters"):
        gp.mfma_probe_lowp(0, n)


@pytest.mark.parametrize("blocks", [0, -1, 1 << 20])
def test_tile_blocks_range(blocks):
    with pytest.raises(ValueError, match="blocks"):
        fp8(blocks=blocks)
    with pytest.raises(ValueError, match="blocks"):
        mx(blocks=blocks)


@pytest.mark.parametrize("blocks", [-1, 1 << 20])
def test_burn_blocks_range(blocks):
    for fmt in ("e4m3", "e2m1"):
        with pytest.raises(ValueError, match="blocks"):
            gp.mfma_mx_burn_run(0, fmt, 1, blocks)


@pytest.mark.parametrize("fmt", ["", "fp8", "E4M3", "e2m3", "e3m2", "e8m0"])
def test_unknown_format(fmt):
    with pytest.raises(ValueError, match="a_fmt"):
        fp8(af=fmt)
    with pytest.raises(ValueError, match="b_fmt"):
        fp8(bf=fmt)
    with pytest.raises(ValueError, match="a_fmt"):
        mx(af=fmt)
    with pytest.raises(ValueError, match="b_fmt"):
        mx(bf=fmt)
    with pytest.raises(ValueError, match="fmt"):
        gp.mfma_mx_burn_run(0, fmt)


def test_formats_of_the_other_entry_points_are_rejected():
    with pytest.raises(ValueError, match="a_fmt"):
        fp8(af="e2m1")                    # fp4 exists only in the scaled form
    with pytest.raises(ValueError, match="b_fmt"):
        fp8(bf="e2m1")
    with pytest.raises(ValueError, match="fmt"):
        gp.mfma_mx_burn_run(0, "e5m2")    # the burn runs e4m3 and e2m1 only


def bad_buffers(shape):
    n = shape[0] * shape[1]
    return [np.zeros(n - 1, np.uint8), np.zeros(n + 1, np.uint8),
            np.zeros(shape, np.int8), np.zeros(shape, np.uint16),
            np.zeros(shape, np.float32), np.zeros(n // 4, np.uint32),
            np.zeros((shape[0], 2 * shape[1]), np.uint8)[:, ::2],
            np.zeros((shape[1], shape[0]), np.uint8).T]


def test_fp8_tile_buffers():
    for a in bad_buffers((16, 32)):
        with pytest.raises(ValueError, match="A_codes must"):
            fp8(A=a)
    for b in bad_buffers((32, 16)):
        with pytest.raises(ValueError, match="B_codes must"):
            fp8(B=b)


def test_mx_tile_buffers():
    for a in bad_buffers((16, 128)):
        with pytest.raises(ValueError, match="A_codes must"):
            mx(A=a)
    for b in bad_buffers((128, 16)):
        with pytest.raises(ValueError, match="B_codes must"):
            mx(B=b)
    for s in bad_buffers((16, 4)):
        with pytest.raises(ValueError, match="A_scales must"):
            mx(sa=s)
    for s in bad_buffers((4, 16)):
        with pytest.raises(ValueError, match="B_scales must"):
            mx(sb=s)
    with pytest.raises(ValueError, match="A_codes must"):
        mx(A=A8)                          # the non-scaled form's tile


@pytest.mark.parametrize("code", [16, 17, 128, 255])
@pytest.mark.parametrize("where", [0, 1000, 2047])
def test_e2m1_code_out_of_range(code, where):
    a = AMX.copy()
    a.reshape(-1)[where] = code
    with pytest.raises(ValueError, match="A_codes.*e2m1"):
        mx(A=a, af="e2m1")
    b = BMX.copy()
    b.reshape(-1)[where] = code
    with pytest.raises(ValueError, match="B_codes.*e2m1"):
        mx(B=b, bf="e2m1", af="e2m1")
