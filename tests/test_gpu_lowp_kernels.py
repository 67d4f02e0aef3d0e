"""GPU-tier tests of the FP8 and block-scaled MX (FP8/FP4) matrix-core
kernels against tests/lowp_ref.py, which shares nothing with the .hip file.

The kernels take row-major element codes and do the lane packing themselves,
so these tests pin the operand maps on hardware:

* decode sweep     — every finite code at every K position, by value;
* k0 identity      — one k at a time, A rows then B columns, bitwise: operand
                     maps (fp4 nibble order included) and the C/D map;
* scale map/sweep  — which E8M0 slot scales which 32 elements, codes 1..254;
* exact random     — tiles whose fp64 product is the f32 answer under any
                     summation order, bitwise, also on 2 blocks per CU;
* general data     — error against fp64, reported (see report_error).

Each test is one launch or at most a few hundred launches of one wave.
"""
import numpy as np
import pytest

import lowp_ref
from lowp_ref import E8M0, code_of, decode, finite_codes, mx_ref
from refnum import bits_f32

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
FP8 = ["e4m3", "e5m2"]
MX = ["e4m3", "e5m2", "e2m1"]
FP8_PAIRS = [(a, b) for a in FP8 for b in FP8]
MX_PAIRS = [("e4m3", "e4m3"), ("e5m2", "e5m2"), ("e2m1", "e2m1"),
            ("e4m3", "e2m1"), ("e2m1", "e5m2")]


def pair_id(p):
    return f"{p[0]}x{p[1]}"


@pytest.fixture(scope="module")
def gp():
    from kata_xpu_device_plugin_amd import _gpuprobe
    if _gpuprobe.device_count() == 0:
        pytest.fail("no GPU visible — these tests require a MI355X")
    return _gpuprobe


@pytest.fixture(scope="module")
def cus(gp):
    return gp.device_info(0)["compute_units"]


def u8(x):
    return np.ascontiguousarray(x, np.uint8)


def run_fp8(gp, A, B, af, bf, blocks=1):
    raw = gp.mfma_fp8_tile_run(0, u8(A), u8(B), af, bf, blocks)
    return np.frombuffer(raw, np.float32).reshape(blocks, 16, 16)


def unit_scales():
    return np.full((16, 4), 127, np.uint8), np.full((4, 16), 127, np.uint8)


def run_mx(gp, A, B, SA, SB, af, bf, blocks=1):
    raw = gp.mfma_mx_tile_run(0, u8(A), u8(B), u8(SA), u8(SB), af, bf, blocks)
    return np.frombuffer(raw, np.float32).reshape(blocks, 16, 16)


def run_form(gp, mx, A, B, af, bf):
    """One block of either form with unit scales."""
    if mx:
        return run_mx(gp, A, B, *unit_scales(), af, bf)[0]
    return run_fp8(gp, A, B, af, bf)[0]


def assert_bits_equal(got, want, what=""):
    g, w = bits_f32(got).reshape(-1), bits_f32(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (
        f"{what}: {bad.size} of {g.size} elements differ; first: " +
        ", ".join(f"[{i}] got {g[i]:#010x} want {w[i]:#010x}" for i in bad[:6]))


def one(fmt):
    return code_of(1.0, fmt)


# --- decode sweep ------------------------------------------------------------

def sweep_codes(fmt):
    """16×16 codes to sweep: code 16i+j for the fp8 formats (NaN and inf
    replaced by 0, since NaN·0 would poison the row), code j for e2m1."""
    if fmt == "e2m1":
        return np.tile(np.arange(16, dtype=np.uint8), (16, 1))
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16)
    keep = np.isin(codes, finite_codes(fmt))
    assert keep.sum() == len(finite_codes(fmt))
    return np.where(keep, codes, 0).astype(np.uint8)


def check_decode_sweep(gp, mx, fmt, other, side):
    K = 128 if mx else 32
    codes = sweep_codes(fmt)
    want = decode(codes, fmt)
    for t in range(K // 16):
        swept = np.zeros((16, K), np.uint8)
        swept[:, 16 * t:16 * t + 16] = codes          # A[i][j+16t] = code(i, j)
        sel = np.zeros((K, 16), np.uint8)
        sel[16 * t + np.arange(16), np.arange(16)] = one(other)   # B[j+16t][j] = 1
        if side == "A":
            D = run_form(gp, mx, swept, sel, fmt, other)
            bad = np.argwhere(D != want)
        else:   # the transposed problem: codes in B, selector in A
            D = run_form(gp, mx, sel.T, swept.T, other, fmt)
            bad = np.argwhere(D != want.T)
        assert bad.size == 0, (fmt, side, t, len(bad), bad[:6], D[tuple(bad[0])])


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("fmt,other", FP8_PAIRS, ids=map(pair_id, FP8_PAIRS))
def test_fp8_decode_sweep(gp, fmt, other, side):
    check_decode_sweep(gp, False, fmt, other, side)


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("fmt,other", [("e4m3", "e4m3"), ("e5m2", "e5m2"),
                                       ("e2m1", "e2m1"), ("e4m3", "e2m1"),
                                       ("e2m1", "e5m2"), ("e5m2", "e4m3")])
def test_mx_decode_sweep(gp, fmt, other, side):
    check_decode_sweep(gp, True, fmt, other, side)


# --- row and column identity, one k at a time -----------------------------------

def distinct_values(fmt):
    """16 exactly representable values, distinct for the fp8 formats. e2m1
    has only 15 distinct values: all of them, zero twice (never -0, so the
    expected bits do not depend on how the hardware signs a zero sum)."""
    i = np.arange(16)
    if fmt == "e4m3":
        return (1 + (i & 7) / 8) * 2.0 ** (i >> 3)
    if fmt == "e5m2":
        return (1 + (i & 3) / 4) * 2.0 ** (i >> 2)
    v = lowp_ref.E2M1.copy()
    v[8] = 0.0
    return v


def check_k0_identity(gp, mx, af, bf):
    K = 128 if mx else 32
    va, vb = distinct_values(af), distinct_values(bf)
    ca = np.array([code_of(v, af) for v in va], np.uint8)
    cb = np.array([code_of(v, bf) for v in vb], np.uint8)
    for k0 in range(K):
        A = np.zeros((16, K), np.uint8)
        B = np.zeros((K, 16), np.uint8)
        A[:, k0], B[k0] = ca, one(bf)
        want = np.repeat(va[:, None], 16, 1).astype(np.float32)
        assert_bits_equal(run_form(gp, mx, A, B, af, bf), want, f"A rows, k0={k0}")
        A[:, k0], B[k0] = one(af), cb
        want = np.repeat(vb[None, :], 16, 0).astype(np.float32)
        assert_bits_equal(run_form(gp, mx, A, B, af, bf), want, f"B columns, k0={k0}")


@pytest.mark.parametrize("af,bf", FP8_PAIRS, ids=map(pair_id, FP8_PAIRS))
def test_fp8_k0_identity(gp, af, bf):
    check_k0_identity(gp, False, af, bf)


@pytest.mark.parametrize("af,bf", MX_PAIRS, ids=map(pair_id, MX_PAIRS))
def test_mx_k0_identity(gp, af, bf):
    check_k0_identity(gp, True, af, bf)


# --- scales --------------------------------------------------------------------

@pytest.mark.parametrize("fmt", MX)
def test_mx_scale_map(gp, fmt):
    """All elements 1; one 32-wide block of one operand is non-zero and its
    16 scale slots hold 127 + (i − 8); every other slot of that operand holds
    127 + 3, which must not show."""
    r = np.arange(16)
    for b in range(4):
        A = np.zeros((16, 128), np.uint8)
        A[:, 32 * b:32 * b + 32] = one(fmt)
        B = np.full((128, 16), one(fmt), np.uint8)
        SA, SB = unit_scales()
        SA[:] = 130
        SA[:, b] = 127 + (r - 8)
        want = np.repeat(32 * 2.0 ** (r - 8)[:, None], 16, 1).astype(np.float32)
        assert_bits_equal(run_mx(gp, A, B, SA, SB, fmt, fmt)[0], want, f"A scales, block {b}")
        # the same for B: D[i][j] = 32·2^(j−8)
        SA, SB = unit_scales()
        SB[:] = 130
        SB[b] = 127 + (r - 8)
        assert_bits_equal(run_mx(gp, B.T, A.T, SA, SB, fmt, fmt)[0], want.T,
                          f"B scales, block {b}")


def scale_sweep_problem(fmt, side, codes):
    """All elements 1. The swept operand's slot (i, b) holds codes[4i + b];
    the other operand is non-zero only where block(k) == j % 4 and all its
    scales are 122 (2^-5, which cancels the 32 equal products). So
    D[i][j] = 2^(codes[4i + j%4] − 127): the E8M0 value itself, normal and
    finite in f32 for every code 1..254, every slot visible."""
    A = np.full((16, 128), one(fmt), np.uint8)
    B = np.zeros((128, 16), np.uint8)
    k, j = np.arange(128)[:, None], np.arange(16)[None, :]
    B[(k // 32) == (j % 4)] = one(fmt)
    SA = np.asarray(codes, np.uint8).reshape(16, 4)
    SB = np.full((4, 16), 122, np.uint8)
    want = E8M0[SA[:, np.arange(16) % 4].astype(np.int64)]
    if side == "A":
        return A, B, SA, SB, want
    return B.T.copy(), A.T.copy(), SB.T.copy(), SA.T.copy(), want.T


@pytest.mark.parametrize("side", ["A", "B"])
def test_mx_scale_sweep(gp, side):
    """E8M0 codes 1..254 through all 64 scale slots of one operand: launch n
    puts code 1 + (n + s) % 254 in slot s, so every slot sees every code."""
    fmt = "e4m3"
    s = np.arange(64)
    for n in range(254):
        A, B, SA, SB, want = scale_sweep_problem(fmt, side, 1 + (n + s) % 254)
        ref, _ = mx_ref(A, B, SA, SB, fmt, fmt)
        assert np.array_equal(ref, want)            # the construction holds
        assert np.all(np.frexp(want)[0] == 0.5)     # exact powers of two
        want = want.astype(np.float32)
        assert np.all(np.isfinite(want)) and np.all(want >= 2.0 ** -126)
        assert_bits_equal(run_mx(gp, A, B, SA, SB, fmt, fmt)[0], want,
                          f"{side} scales, launch {n}")


def test_mx_scale_codes_0_and_255_reported(gp):
    """What the hardware returns for E8M0 0 (2^-127) and 255 (NaN in the MX
    specification) is printed, not asserted."""
    fmt = "e4m3"
    A = np.full((16, 128), one(fmt), np.uint8)
    B = np.full((128, 16), one(fmt), np.uint8)
    for code in (0, 255):
        SA, SB = unit_scales()
        SA[:] = code
        D = run_mx(gp, A, B, SA, SB, fmt, fmt)[0]
        print(f"E8M0 code {code} on A (all-ones K=128, B scale 127): "
              f"D[0][0] = {D[0, 0]!r} bits {bits_f32(D)[0, 0]:#010x}, "
              f"{np.unique(bits_f32(D)).size} distinct values")


# --- exact data ------------------------------------------------------------------

EXP_FIELD = {"e4m3": (6, 3), "e5m2": (14, 2)}       # lowest exponent field, mantissa bits
SCALE_RANGE = {"e4m3": (127, 128), "e5m2": (127, 128), "e2m1": (125, 129)}


def exact_codes(rng, fmt, shape):
    """Random sign and mantissa with the exponent field in a window of four
    (e4m3: 6..9, e5m2: 14..17); e2m1: all 16 codes."""
    if fmt == "e2m1":
        return rng.integers(0, 16, shape).astype(np.uint8)
    lo, mbits = EXP_FIELD[fmt]
    sign = rng.integers(0, 2, shape) << 7
    exp = rng.integers(lo, lo + 4, shape) << mbits
    return (sign | exp | rng.integers(0, 1 << mbits, shape)).astype(np.uint8)


def smallest_step(fmt, scaled):
    """Smallest spacing of the values exact_codes() draws, times the smallest
    scale exact_scales() draws."""
    step = {"e4m3": 2.0 ** (6 - 7 - 3), "e5m2": 2.0 ** (14 - 15 - 2), "e2m1": 0.5}[fmt]
    return step * (2.0 ** (SCALE_RANGE[fmt][0] - 127) if scaled else 1.0)


def exact_scales(rng, fmt, shape):
    lo, hi = SCALE_RANGE[fmt]
    return rng.integers(lo, hi + 1, shape).astype(np.uint8)


def exact_mx_problem(seed, af, bf):
    rng = np.random.default_rng(seed)
    A, B = exact_codes(rng, af, (16, 128)), exact_codes(rng, bf, (128, 16))
    SA, SB = exact_scales(rng, af, (16, 4)), exact_scales(rng, bf, (4, 16))
    ref, mag = mx_ref(A, B, SA, SB, af, bf)
    quantum = smallest_step(af, True) * smallest_step(bf, True)
    # every product is a multiple of quantum and every partial sum is below
    # 2^24 quanta: the fp64 product is the f32 answer under any order
    assert np.all(ref / quantum == np.round(ref / quantum))
    assert mag.max() / quantum < 2.0 ** 24
    print(f"exact MX {af}x{bf} seed {seed}: max Σ|a·b|/quantum = "
          f"2^{np.log2(mag.max() / quantum):.1f}")
    want = ref.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref)
    return A, B, SA, SB, want


def exact_fp8_problem(seed, af, bf):
    rng = np.random.default_rng(seed)
    A, B = exact_codes(rng, af, (16, 32)), exact_codes(rng, bf, (32, 16))
    a, b = decode(A, af), decode(B, bf)
    ref, mag = a @ b, np.abs(a) @ np.abs(b)
    quantum = smallest_step(af, False) * smallest_step(bf, False)
    assert np.all(ref / quantum == np.round(ref / quantum))
    assert mag.max() / quantum < 2.0 ** 24
    want = ref.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref)
    return A, B, want


@pytest.mark.parametrize("seed", [200, 201, 202])
@pytest.mark.parametrize("af,bf", FP8_PAIRS, ids=map(pair_id, FP8_PAIRS))
def test_fp8_exact_random(gp, af, bf, seed):
    A, B, want = exact_fp8_problem(seed, af, bf)
    assert_bits_equal(run_fp8(gp, A, B, af, bf)[0], want, f"{af}x{bf} seed {seed}")


@pytest.mark.parametrize("seed", [200, 201, 202])
@pytest.mark.parametrize("af,bf", MX_PAIRS, ids=map(pair_id, MX_PAIRS))
def test_mx_exact_random(gp, af, bf, seed):
    A, B, SA, SB, want = exact_mx_problem(seed, af, bf)
    assert_bits_equal(run_mx(gp, A, B, SA, SB, af, bf)[0], want, f"{af}x{bf} seed {seed}")


def assert_slabs_equal(D):
    bad = [b for b in range(1, len(D)) if not np.array_equal(bits_f32(D[b]), bits_f32(D[0]))]
    assert not bad, f"slabs differing from slab 0: {bad[:16]}"


def test_fp8_exact_every_cu(gp, cus):
    A, B, want = exact_fp8_problem(200, "e4m3", "e4m3")
    D = run_fp8(gp, A, B, "e4m3", "e4m3", blocks=2 * cus)
    assert_bits_equal(D[0], want, "slab 0")
    assert_slabs_equal(D)


@pytest.mark.parametrize("fmt", ["e4m3", "e2m1"])
def test_mx_exact_every_cu(gp, cus, fmt):
    A, B, SA, SB, want = exact_mx_problem(200, fmt, fmt)
    D = run_mx(gp, A, B, SA, SB, fmt, fmt, blocks=2 * cus)
    assert_bits_equal(D[0], want, "slab 0")
    assert_slabs_equal(D)


@pytest.mark.parametrize("af,bf", FP8_PAIRS, ids=map(pair_id, FP8_PAIRS))
def test_mx_unit_scales_reproduce_unscaled_product(gp, af, bf):
    """One 32-wide K-slice, the rest zero, scales 127: bit for bit the
    non-scaled 16x16x32 instruction's result on exact data. On full-range
    data, where the two instructions' internal rounding could differ, the
    number of differing elements is printed and not asserted."""
    for b in range(4):
        A32, B32, want = exact_fp8_problem(210 + b, af, bf)
        A = np.zeros((16, 128), np.uint8)
        B = np.zeros((128, 16), np.uint8)
        A[:, 32 * b:32 * b + 32], B[32 * b:32 * b + 32] = A32, B32
        D8 = run_fp8(gp, A32, B32, af, bf)[0]
        Dmx = run_form(gp, True, A, B, af, bf)
        assert_bits_equal(Dmx, D8, f"block {b}")
        assert_bits_equal(Dmx, want, f"block {b} vs host")
    rng = np.random.default_rng(214)
    A32 = rng.choice(finite_codes(af), (16, 32))
    B32 = rng.choice(finite_codes(bf), (32, 16))
    A = np.zeros((16, 128), np.uint8)
    B = np.zeros((128, 16), np.uint8)
    A[:, :32], B[:32] = A32, B32
    differ = np.count_nonzero(bits_f32(run_form(gp, True, A, B, af, bf)) !=
                              bits_f32(run_fp8(gp, A32, B32, af, bf)[0]))
    print(f"full-range {af}x{bf}: MX at unit scales differs from the non-scaled "
          f"form in {differ} of 256 elements")


# --- general data ------------------------------------------------------------------

def report_error(D, a, b, K, what):
    """Error of D against the fp64 product of the (scaled) operand values, in
    units of K·2^-23·Σ|a·b| — the bound that would hold if products were
    exact and each of the K additions lost at most one f32 ulp — and as a
    fraction of the largest single product of each element.

    Measured on an MI355X, full-range random codes, seeds 0..2: the
    non-scaled 16x16x32 forms reach 28.4..51.9 times that bound and the
    scaled 16x16x128 form (scales 119..135) 5.5..13.7 times; the worst error
    is 2^-11.4..2^-12.9 of the largest product in both. So the matrix core
    does not keep a full-width sum of these formats' products. The bound
    is therefore not asserted (and not widened by guess); what is asserted on
    general data is only that the result is finite. The probes' `ok` rests on
    the exact tiles alone. docs/testing.md records the figures."""
    ref, mag = a @ b, np.abs(a) @ np.abs(b)
    peak = (np.abs(a)[:, :, None] * np.abs(b)[None, :, :]).max(axis=1)
    err = np.abs(D.astype(np.float64) - ref)
    print(f"{what}: worst error/(K·2^-23·Σ|a·b|) = {(err / (K * EPS * mag)).max():.4f}, "
          f"worst error/max|a·b| = 2^{np.log2((err / peak).max()):.2f}")
    assert np.all(np.isfinite(D))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("af,bf", FP8_PAIRS, ids=map(pair_id, FP8_PAIRS))
def test_fp8_general_error_reported(gp, af, bf, seed):
    rng = np.random.default_rng(300 + seed)
    A = rng.choice(finite_codes(af), (16, 32))
    B = rng.choice(finite_codes(bf), (32, 16))
    report_error(run_fp8(gp, A, B, af, bf)[0], decode(A, af), decode(B, bf), 32,
                 f"fp8 {af}x{bf} seed {seed}")


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("af,bf", FP8_PAIRS, ids=map(pair_id, FP8_PAIRS))
def test_mx_general_error_reported(gp, af, bf, seed):
    rng = np.random.default_rng(400 + seed)
    A = rng.choice(finite_codes(af), (16, 128))
    B = rng.choice(finite_codes(bf), (128, 16))
    SA = rng.integers(119, 136, (16, 4)).astype(np.uint8)
    SB = rng.integers(119, 136, (4, 16)).astype(np.uint8)
    a = decode(A, af) * np.repeat(E8M0[SA.astype(np.int64)], 32, axis=1)
    b = decode(B, bf) * np.repeat(E8M0[SB.astype(np.int64)], 32, axis=0)
    report_error(run_mx(gp, A, B, SA, SB, af, bf)[0], a, b, 128,
                 f"MX {af}x{bf} seed {seed}")


# --- NaN -----------------------------------------------------------------------------

@pytest.mark.parametrize("mx", [False, True], ids=["fp8", "mx"])
def test_nan_stays_in_its_row(gp, mx):
    K = 128 if mx else 32
    rng = np.random.default_rng(5)
    ints = np.array([code_of(float(v), "e4m3") for v in range(-4, 5)], np.uint8)
    A, B = rng.choice(ints, (16, K)), rng.choice(ints, (K, 16))
    want = (decode(A, "e4m3") @ decode(B, "e4m3")).astype(np.float32)
    row = 7
    A[row, K - 3] = 0x7F
    D = run_form(gp, mx, A, B, "e4m3", "e4m3")
    others = np.arange(16) != row
    assert np.all(np.isnan(D[row])), D[row]
    assert_bits_equal(D[others], want[others], "rows without NaN")


# --- burn ----------------------------------------------------------------------------

def lane_k(fmt, g, e):
    """k of element e of lane group g, as the tests above pin it: fp4 lanes
    hold one 32-wide block, fp8 lanes two 16-wide runs 64 apart."""
    if fmt == "e2m1":
        return 32 * g + e
    return 64 * (e >> 4) + 16 * g + (e & 15)


def mx_burn_model(fmt, iters):
    """The burn kernel's data formulas through the pinned maps: element e of
    lane l is 1 + (l+e)%3 in A[l&15][k] and 1 + (l^e)%3 in B[k][l&15],
    k = lane_k(l>>4, e); accumulator n of 8 starts at n; lane l stores
    Σ_n Σ_reg acc_n[reg] with reg ↔ D[4(l>>4)+reg][l&15]."""
    l, e = np.arange(64)[:, None], np.arange(32)[None, :]
    A = np.zeros((16, 128), np.int64)
    B = np.zeros((128, 16), np.int64)
    k = lane_k(fmt, l >> 4, e)
    A[l & 15, k] = 1 + (l + e) % 3
    B[k, l & 15] = 1 + (l ^ e) % 3
    assert A.min() >= 1 and B.min() >= 1            # every element written
    D = A @ B
    lanes = np.array([sum(n + iters * D[4 * (l >> 4) + reg, l & 15]
                          for n in range(8) for reg in range(4)) for l in range(64)])
    assert lanes.max() < 2 ** 24
    return lanes.astype(np.float32)


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("fmt", ["e4m3", "e2m1"])
def test_mx_burn_lanes_match_model(gp, fmt, iters):
    r = gp.mfma_mx_burn_run(0, fmt, iters, 2)
    assert r["blocks"] == 2 and r["mismatches"] == 0, r
    lanes = np.frombuffer(r["lanes"], np.float32)
    want = mx_burn_model(fmt, iters)
    assert np.unique(want).size > 8            # the data varies by lane
    assert_bits_equal(lanes, want, f"{fmt} iters={iters}")


@pytest.mark.parametrize("fmt", ["e4m3", "e2m1"])
def test_mx_burn_every_wave_agrees(gp, cus, fmt):
    r = gp.mfma_mx_burn_run(0, fmt, 3)
    assert r["blocks"] == 2 * cus
    assert r["mismatches"] == 0, r["mismatches"]


# --- probe ----------------------------------------------------------------------------

FORMS = ("fp8", "mx_fp8", "mx_fp4")


def test_probe_lowp_healthy(gp):
    r = gp.mfma_probe_lowp(0, 2000)
    for form in FORMS:
        assert r[f"{form}_ok"] is True, (form, r)
        assert r[f"{form}_slab_mismatches"] == 0, (form, r)
    for form in FORMS[1:]:
        assert r[f"{form}_burn_mismatches"] == 0, (form, r)
        assert r[f"{form}_tflops"] > 0 and r[f"{form}_burn_ms"] > 0, (form, r)


def test_probe_lowp_rates_above_floors(gp):
    from kata_xpu_device_plugin_amd.health import gpuprobe
    r = gp.mfma_probe_lowp(0, 20000)
    print(f"MX-fp8 {r['mx_fp8_tflops']:.0f} TF in {r['mx_fp8_burn_ms']:.2f} ms, "
          f"MX-fp4 {r['mx_fp4_tflops']:.0f} TF in {r['mx_fp4_burn_ms']:.2f} ms")
    assert r["mx_fp8_tflops"] >= gpuprobe.MX_FP8_TFLOPS_FLOOR_MI355X, r
    assert r["mx_fp4_tflops"] >= gpuprobe.MX_FP4_TFLOPS_FLOOR_MI355X, r
    assert r["mx_fp8_burn_mismatches"] == r["mx_fp4_burn_mismatches"] == 0, r


def test_probe_device_low_precision():
    from kata_xpu_device_plugin_amd.health.gpuprobe import probe_device
    rep = probe_device(0, bandwidth_bytes=256 << 20, memtest_bytes=256 << 20,
                       burn_iters=4000, low_precision=True)
    assert rep.passed, rep.failures
    assert rep.mfma_fp8_ok and rep.mfma_mx_fp8_ok and rep.mfma_mx_fp4_ok
    assert rep.mx_fp8_tflops > 0 and rep.mx_fp4_tflops > 0
    for f in ("mfma_fp8_slab_mismatches", "mfma_mx_fp8_slab_mismatches",
              "mfma_mx_fp4_slab_mismatches", "mx_fp8_burn_mismatches",
              "mx_fp4_burn_mismatches"):
        assert getattr(rep, f) == 0, (f, rep.as_dict())
