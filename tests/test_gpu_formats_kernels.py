"""GPU-tier tests of the FP64 / FP16 / INT8 / 2:4-sparse matrix-core kernels of
_gpuprobe_formats against tests/formats_ref.py, which shares nothing with the
.hip file.

The kernels take row-major operands and do the lane packing themselves, so
these tests pin the lane maps on hardware:

* one k at a time — distinct values down one column of A against a row of
                    ones and the reverse, bitwise: operand maps and C/D map;
* selector        — identity-like A against an asymmetric B (row↔column, and
                    the f64 form's own row formula);
* sparse slots    — a single 1 per row of the kept A at every slot and index
                    value: slot→group, index bit position and the B map;
* exact data      — tiles whose product is the answer under any summation
                    order, bitwise, also on 2 blocks per CU;
* general data    — error against the exact sum, within a derived bound.

Every case is one wave per block at blocks = 1, at most a few hundred
launches, plus one 2 × CUs launch per form.
"""
from fractions import Fraction

import numpy as np
import pytest

import formats_ref as fr
from refnum import bits_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gf():
    from kata_xpu_device_plugin_amd import _gpuprobe, _gpuprobe_formats
    if _gpuprobe.device_count() == 0:
        pytest.fail("no GPU visible — these tests require a MI355X")
    return _gpuprobe_formats


@pytest.fixture(scope="module")
def cus():
    from kata_xpu_device_plugin_amd import _gpuprobe
    return _gpuprobe.device_info(0)["compute_units"]


def run_f64(gf, A, B, C=None, blocks=1):
    c = None if C is None else np.ascontiguousarray(C, np.float64)
    raw = gf.mfma_f64_tile_run(0, np.ascontiguousarray(A, np.float64),
                               np.ascontiguousarray(B, np.float64), c, blocks)
    return np.frombuffer(raw, np.float64).reshape(blocks, 16, 16)


def run_f16(gf, A_bits, B_bits, blocks=1):
    raw = gf.mfma_f16_tile_run(0, np.ascontiguousarray(A_bits, np.uint16),
                               np.ascontiguousarray(B_bits, np.uint16), blocks)
    return np.frombuffer(raw, np.float32).reshape(blocks, 32, 32)


def run_i8(gf, A, B, C=None, blocks=1):
    c = None if C is None else np.ascontiguousarray(C, np.int32)
    raw = gf.mfma_i8_tile_run(0, np.ascontiguousarray(A, np.int8),
                              np.ascontiguousarray(B, np.int8), c, blocks)
    return np.frombuffer(raw, np.int32).reshape(blocks, 16, 16)


def run_sp(gf, A_bits, idx, B_bits, blocks=1):
    raw = gf.smfmac_f16_tile_run(0, np.ascontiguousarray(A_bits, np.uint16),
                                 np.ascontiguousarray(idx, np.uint8),
                                 np.ascontiguousarray(B_bits, np.uint16), blocks)
    return np.frombuffer(raw, np.float32).reshape(blocks, 16, 16)


def assert_bits_equal(got, want, what=""):
    """Bitwise comparison of two arrays of one dtype (f32, f64 or i32)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g, w = got.view(u).reshape(-1), want.view(u).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (
        f"{what}: {bad.size} of {g.size} elements differ; first: " +
        ", ".join(f"[{i}] got {int(g[i]):#x} want {int(w[i]):#x}" for i in bad[:6]))


def assert_slabs_equal(D):
    flat = np.ascontiguousarray(D).reshape(len(D), -1).view(np.uint8)
    bad = [b for b in range(1, len(D)) if not np.array_equal(flat[b], flat[0])]
    assert not bad, f"slabs differing from slab 0: {bad[:16]}"


# --- f64: layout -------------------------------------------------------------

# 16 distinct full-mantissa values over 16 binades
F64_VALS = (1 + np.arange(16) / 17.0) * 2.0 ** np.arange(-8, 8)


def test_f64_one_k_at_a_time(gf):
    for k in range(4):
        A, B = np.zeros((16, 4)), np.zeros((4, 16))
        A[:, k], B[k] = F64_VALS, 1.0
        assert_bits_equal(run_f64(gf, A, B)[0], np.repeat(F64_VALS[:, None], 16, 1),
                          f"A rows, k={k}")
        A[:, k], B[k] = 1.0, F64_VALS
        assert_bits_equal(run_f64(gf, A, B)[0], np.repeat(F64_VALS[None, :], 16, 0),
                          f"B columns, k={k}")


def test_f64_selector_against_asymmetric_b(gf):
    """A[i][i%4] = i+1, B[k][j] = 100k + j + 0.5: D[i][j] = (i+1)·B[i%4][j],
    16 distinct rows, no symmetry. The f32 row formula 4(l>>4)+r on this
    instruction would put 3 of every 4 rows in the wrong place."""
    A = np.zeros((16, 4))
    A[np.arange(16), np.arange(16) % 4] = np.arange(16) + 1.0
    B = 100.0 * np.arange(4)[:, None] + np.arange(16)[None, :] + 0.5
    want = (np.arange(16) + 1.0)[:, None] * B[np.arange(16) % 4]
    assert not np.array_equal(want, want.T)
    assert_bits_equal(run_f64(gf, A, B)[0], want, "selector")


def test_f64_c_passes_through(gf):
    rng = np.random.default_rng(10)
    C = rng.standard_normal((16, 16)) * 2.0 ** rng.integers(-300, 300, (16, 16))
    assert_bits_equal(run_f64(gf, np.zeros((16, 4)), np.zeros((4, 16)), C)[0], C, "C")


# --- f64: numerics --------------------------------------------------------------

def f64_exact_problem(seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-2 ** 20, 2 ** 20, (16, 4)).astype(np.float64)
    B = rng.integers(-2 ** 20, 2 ** 20, (4, 16)).astype(np.float64)
    C = rng.integers(-2 ** 40, 2 ** 40, (16, 16)).astype(np.float64)
    want = (A.astype(np.int64) @ B.astype(np.int64) + C.astype(np.int64))
    assert np.abs(want).max() < 2 ** 53
    return A, B, C, want.astype(np.float64)


@pytest.mark.parametrize("seed", [20, 21, 22])
def test_f64_exact_integer_random(gf, seed):
    A, B, C, want = f64_exact_problem(seed)
    assert_bits_equal(run_f64(gf, A, B, C)[0], want, f"seed {seed}")
    assert_bits_equal(run_f64(gf, A, B)[0], want - C, f"seed {seed}, no C")


def test_f64_exact_every_cu(gf, cus):
    A, B, C, want = f64_exact_problem(20)
    D = run_f64(gf, A, B, C, blocks=2 * cus)
    assert_bits_equal(D[0], want, "slab 0")
    assert_slabs_equal(D)


def test_f64_signed_zero(gf):
    """Sums whose sign does not depend on the order: every term -0 gives -0;
    a +0 product added to a -0 C gives +0 (round to nearest)."""
    A, B = np.full((16, 4), -0.0), np.full((4, 16), 3.0)
    negz = np.full((16, 16), -0.0)
    assert_bits_equal(run_f64(gf, A, B, negz)[0], negz, "(-0)·3 + (-0)")
    assert_bits_equal(run_f64(gf, -A, B, negz)[0], -negz, "(+0)·3 + (-0)")
    assert_bits_equal(fr.mfma_f64_chain(A, B, negz), negz, "reference")


def test_f64_subnormals(gf):
    """Subnormal inputs, subnormal products of normal inputs and a subnormal
    C, all multiples of 2^-1074 with sums far below 2^53 steps: exact in any
    order, and nothing is flushed."""
    i, k, j = np.arange(16)[:, None], np.arange(4)[None, :], np.arange(16)[None, :]
    tiny = 2.0 ** -1074
    A = (1 + i + 5 * k) * tiny * 2.0 ** 10                    # subnormal inputs
    B = (np.arange(4)[:, None] + 1.0) * 2.0 ** (j % 8)
    C = (i * 16 + j + 1) * tiny
    want = np.array([[sum(Fraction(float(A[a, c])) * Fraction(float(B[c, b])) for c in range(4))
                      + Fraction(float(C[a, b])) for b in range(16)] for a in range(16)])
    want = np.array([[float(x) for x in row] for row in want])
    assert 0 < want.max() < 2.0 ** -1022                       # still subnormal
    assert_bits_equal(run_f64(gf, A, B, C)[0], want, "subnormal inputs and C")
    A2 = (2 * i + 2 * k + 1) * 2.0 ** -600                     # normal · normal → subnormal
    B2 = (2 * np.arange(4)[:, None] + j + 1) * 2.0 ** -470
    want2 = (A2 * 2.0 ** 600) @ (B2 * 2.0 ** 470) * 2.0 ** -1070
    assert 0 < want2.max() < 2.0 ** -1022
    assert_bits_equal(run_f64(gf, A2, B2)[0], want2, "subnormal products")


def test_f64_inf_and_nan_stay_in_their_row_or_column(gf):
    A, B, C, want = f64_exact_problem(23)
    A, B = np.abs(A) + 1, np.abs(B) + 1                        # no 0·inf, no inf-inf
    want = A @ B + C
    A[3, 1] = np.inf
    B[2, 5] = -np.inf
    A[7, 0] = np.nan
    D = run_f64(gf, A, B, C)[0]
    clean = np.ones((16, 16), bool)
    clean[[3, 7]] = False
    clean[:, 5] = False
    assert_bits_equal(D[clean], want[clean], "untouched elements")
    assert np.all(np.isnan(D[7]))
    assert np.all(D[3, np.arange(16) != 5] == np.inf) and np.isnan(D[3, 5])
    assert np.all(D[np.setdiff1d(np.arange(16), [3, 7]), 5] == -np.inf)


@pytest.mark.parametrize("seed", [30, 31, 32])
def test_f64_full_mantissa_within_bound(gf, seed):
    """|D − exact| ≤ 8·2^-53·(|c| + Σ|a·b|): four products and four sums, each
    rounded at most once at no more than the total magnitude, so the bound
    holds fused or not and in any order. Whether the result is the k-ordered
    once-rounded chain bit for bit is printed, not asserted."""
    rng = np.random.default_rng(seed)
    def draw(shape):
        return rng.uniform(1, 2, shape) * rng.choice([-1.0, 1.0], shape) * \
            2.0 ** rng.integers(-4, 4, shape)
    A, B, C = draw((16, 4)), draw((4, 16)), draw((16, 16))
    D = run_f64(gf, A, B, C)[0]
    assert np.all(np.isfinite(D))
    total, mag = fr.mfma_f64_exact(A, B, C)
    ratio = max(abs(Fraction(float(D[i, j])) - total[i][j]) /
                (8 * Fraction(2) ** -53 * mag[i][j]) for i in range(16) for j in range(16))
    chain = fr.mfma_f64_chain(A, B, C)
    differ = np.count_nonzero(fr.bits_f64(D) != fr.bits_f64(chain))
    print(f"f64 seed {seed}: worst error/bound = {float(ratio):.4f}; differs from the "
          f"k-ordered fma chain in {differ} of 256 elements")
    assert ratio <= 1, float(ratio)


# --- f16 ------------------------------------------------------------------------

# 32 distinct f16 values: (1 + m/8)·2^e
F16_VALS = (1 + (np.arange(32) & 7) / 8) * 2.0 ** (np.arange(32) >> 3)
ONE16 = 0x3C00


def test_f16_one_k_at_a_time(gf):
    vals = fr.f16_bits(F16_VALS)
    for k in range(16):
        A, B = np.zeros((32, 16), np.uint16), np.zeros((16, 32), np.uint16)
        A[:, k], B[k] = vals, ONE16
        assert_bits_equal(run_f16(gf, A, B)[0],
                          np.repeat(F16_VALS[:, None], 32, 1).astype(np.float32),
                          f"A rows, k={k}")
        A[:, k], B[k] = ONE16, vals
        assert_bits_equal(run_f16(gf, A, B)[0],
                          np.repeat(F16_VALS[None, :], 32, 0).astype(np.float32),
                          f"B columns, k={k}")


def f16_exact_problem(seed):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(-16, 17, (32, 16)), rng.integers(-16, 17, (16, 32))
    return fr.f16_bits(a), fr.f16_bits(b), (a @ b).astype(np.float32)


@pytest.mark.parametrize("seed", [40, 41, 42])
def test_f16_integer_tiles(gf, seed):
    A, B, want = f16_exact_problem(seed)
    ref, _ = fr.mfma_f16_ref(A, B)
    assert np.array_equal(ref, want)
    assert_bits_equal(run_f16(gf, A, B)[0], want, f"seed {seed}")


def test_f16_exact_every_cu(gf, cus):
    A, B, want = f16_exact_problem(40)
    D = run_f16(gf, A, B, blocks=2 * cus)
    assert_bits_equal(D[0], want, "slab 0")
    assert_slabs_equal(D)


def test_f16_subnormal_and_max_normal_inputs(gf):
    """Products of f16 values fit f32 exactly. Subnormal codes 1..1023
    (c·2^-24) against integers in -4..4: every sum is a multiple of 2^-24
    below 2^16 of them. Max-normal 65504² = 2047²·2^10: one product per
    output element."""
    rng = np.random.default_rng(43)
    A = rng.integers(1, 1024, (32, 16)).astype(np.uint16)
    A |= (rng.integers(0, 2, (32, 16)) << 15).astype(np.uint16)
    b = rng.integers(-4, 5, (16, 32))
    ref, _ = fr.mfma_f16_ref(A, fr.f16_bits(b))
    want = ref.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref) and np.abs(ref).max() < 2.0 ** -8
    assert_bits_equal(run_f16(gf, A, fr.f16_bits(b))[0], want, "subnormal A")
    assert_bits_equal(run_f16(gf, fr.f16_bits(b.T), A.T.copy())[0], want.T, "subnormal B")
    A = np.zeros((32, 16), np.uint16)
    A[np.arange(32), np.arange(32) % 16] = 0x7BFF
    sign = (np.add.outer(np.arange(16), np.arange(32)) % 3 == 0)
    B = np.where(sign, 0xFBFF, 0x7BFF).astype(np.uint16)
    ref, _ = fr.mfma_f16_ref(A, B)
    want = ref.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref) and np.abs(ref).max() == 65504.0 ** 2
    assert_bits_equal(run_f16(gf, A, B)[0], want, "max normal")


def test_f16_nan_stays_in_its_row(gf):
    A, B, want = f16_exact_problem(44)
    A[9, 13] = 0x7E00
    D = run_f16(gf, A, B)[0]
    others = np.arange(32) != 9
    assert np.all(np.isnan(D[9])), D[9]
    assert_bits_equal(D[others], want[others], "rows without NaN")


@pytest.mark.parametrize("seed", [50, 51, 52])
def test_f16_random_within_bound(gf, seed):
    """Each f16×f16 product has at most 22 significant bits and is exact in
    f32; 16 additions lose at most one ulp each in any order (the bf16 tile's
    argument): |D − ref| ≤ 16·2^-23·Σ|a·b|."""
    rng = np.random.default_rng(seed)
    def draw(shape):
        sign = rng.integers(0, 2, shape) << 15
        return (sign | rng.integers(11, 19, shape) << 10 |
                rng.integers(0, 1024, shape)).astype(np.uint16)
    A, B = draw((32, 16)), draw((16, 32))
    D = run_f16(gf, A, B)[0]
    ref, mag = fr.mfma_f16_ref(A, B)
    ratio = (np.abs(D.astype(np.float64) - ref) / (16 * 2.0 ** -23 * mag)).max()
    print(f"f16 seed {seed}: worst error/(16·2^-23·Σ|a·b|) = {ratio:.4f}")
    assert np.all(np.isfinite(D))
    assert ratio <= 1, ratio


# --- i8 ------------------------------------------------------------------------------

I8_VALS = np.array([-128, -127, -100, -64, -33, -8, -2, -1, 1, 2, 7, 31, 63, 99, 126, 127])


def test_i8_one_k_at_a_time(gf):
    """Settles the operand map as far as a product can: every k of the
    row-major operands reaches the same k of the other one."""
    for k in range(64):
        A, B = np.zeros((16, 64), np.int8), np.zeros((64, 16), np.int8)
        A[:, k], B[k] = I8_VALS, 1
        assert_bits_equal(run_i8(gf, A, B)[0],
                          np.repeat(I8_VALS[:, None], 16, 1).astype(np.int32), f"A rows, k={k}")
        A[:, k], B[k] = 1, I8_VALS
        assert_bits_equal(run_i8(gf, A, B)[0],
                          np.repeat(I8_VALS[None, :], 16, 0).astype(np.int32),
                          f"B columns, k={k}")


def test_i8_extremes_at_every_k(gf):
    ext = np.where(np.arange(16) % 2 == 0, -128, 127)
    for k in range(64):
        A, B = np.zeros((16, 64), np.int8), np.zeros((64, 16), np.int8)
        A[:, k], B[k] = ext, ext[::-1]
        assert_bits_equal(run_i8(gf, A, B)[0], np.outer(ext, ext[::-1]).astype(np.int32),
                          f"k={k}")
    A, B = np.full((16, 64), -128, np.int8), np.full((64, 16), -128, np.int8)
    assert_bits_equal(run_i8(gf, A, B)[0], np.full((16, 16), 2 ** 20, np.int32), "all -128")


def i8_problem(seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-128, 128, (16, 64)).astype(np.int8)
    B = rng.integers(-128, 128, (64, 16)).astype(np.int8)
    C = rng.integers(-2 ** 30, 2 ** 30, (16, 16)).astype(np.int32)
    return A, B, C


@pytest.mark.parametrize("seed", [60, 61, 62])
def test_i8_full_range_random(gf, seed):
    A, B, C = i8_problem(seed)
    assert_bits_equal(run_i8(gf, A, B)[0], fr.mfma_i8_ref(A, B), f"seed {seed}")
    assert_bits_equal(run_i8(gf, A, B, C)[0], fr.mfma_i8_ref(A, B, C), f"seed {seed} with C")


def test_i8_exact_every_cu(gf, cus):
    A, B, C = i8_problem(60)
    D = run_i8(gf, A, B, C, blocks=2 * cus)
    assert_bits_equal(D[0], fr.mfma_i8_ref(A, B, C), "slab 0")
    assert_slabs_equal(D)


def test_i8_accumulator_overflow_reported(gf):
    """An accumulator near INT32_MAX plus a positive product: whether the
    hardware wraps or saturates is printed, not asserted."""
    A, B = np.full((16, 64), 127, np.int8), np.full((64, 16), 127, np.int8)
    C = np.full((16, 16), 2 ** 31 - 6, np.int32)
    D = run_i8(gf, A, B, C)[0]
    wrapped = fr.mfma_i8_ref(A, B, C)
    kind = ("wraps" if np.array_equal(D, wrapped) else
            "saturates" if np.all(D == 2 ** 31 - 1) else "neither wraps nor saturates")
    print(f"i8 accumulator overflow: INT32_MAX-5 + 64·127² gives {int(D[0, 0])} "
          f"(wrap would be {int(wrapped[0, 0])}): {kind}")


# --- 2:4 sparse -----------------------------------------------------------------------

# rows distinct, columns asymmetric, every value an integer exact in f16
SP_B = (np.arange(64)[:, None] * 16 + np.arange(16)[None, :] + 1).astype(np.float64)


def test_sparse_every_slot_and_index_value(gf):
    """Launch (e, v): row i of the kept A holds a single 1, at slot
    (e + i) % 32 with index (v + i) % 4, so every row tests another slot and
    index value at once and D[i][:] must be row 4(slot>>1)+index of B. The
    index values of the empty slots differ from launch to launch and must not
    matter. Pins slot → group, the index bit position and the B map."""
    B = fr.f16_bits(SP_B)
    i = np.arange(16)
    for e in range(32):
        for v in range(4):
            slot, pos = (e + i) % 32, (v + i) % 4
            A = np.zeros((16, 32), np.uint16)
            A[i, slot] = ONE16
            idx = np.full((16, 32), (e + v) % 4, np.uint8)
            idx[i, slot] = pos
            want = SP_B[4 * (slot >> 1) + pos].astype(np.float32)
            assert_bits_equal(run_sp(gf, A, idx, B)[0], want, f"slot {e}, index {v}")


def sparse_problem(seed, zero_fraction=0.0):
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 17, (16, 32)) * rng.choice([-1, 1], (16, 32))
    a[rng.random((16, 32)) < zero_fraction] = 0
    b = rng.integers(-16, 17, (64, 16))
    # every group column holds all six ascending pairs over the 16 rows
    pair = (np.arange(16)[:, None] + np.arange(16)[None, :] + rng.integers(0, 6)) % 6
    idx = np.array(fr.INDEX_PAIRS, np.uint8)[pair].reshape(16, 32)
    assert all(len(set(map(tuple, idx[:, 2 * g:2 * g + 2].tolist()))) == 6 for g in range(16))
    return fr.f16_bits(a), idx, fr.f16_bits(b)


@pytest.mark.parametrize("seed", [70, 71, 72])
def test_sparse_all_index_pairs_exact(gf, seed):
    A, idx, B = sparse_problem(seed)
    ref, mag = fr.smfmac_f16_ref(A, idx, B)
    assert mag.max() < 2 ** 24
    assert_bits_equal(run_sp(gf, A, idx, B)[0], ref.astype(np.float32), f"seed {seed}")


def test_sparse_kept_zeros(gf):
    A, idx, B = sparse_problem(73, zero_fraction=0.4)
    assert np.count_nonzero(A == 0) > 100
    ref, _ = fr.smfmac_f16_ref(A, idx, B)
    assert_bits_equal(run_sp(gf, A, idx, B)[0], ref.astype(np.float32), "kept zeros")


def test_sparse_exact_every_cu(gf, cus):
    A, idx, B = sparse_problem(70)
    ref, _ = fr.smfmac_f16_ref(A, idx, B)
    D = run_sp(gf, A, idx, B, blocks=2 * cus)
    assert_bits_equal(D[0], ref.astype(np.float32), "slab 0")
    assert_slabs_equal(D)


def test_sparse_reversed_and_equal_pairs_reported(gf):
    """2:4 metadata is normally ascending within a group. What the hardware
    does with a descending or a repeated position is printed, not asserted."""
    A, _, B = sparse_problem(74)
    for name, pairs in (("descending", [(b, a) for a, b in fr.INDEX_PAIRS]),
                        ("equal", [(0, 0), (1, 1), (2, 2), (3, 3), (0, 0), (3, 3)])):
        pair = (np.arange(16)[:, None] + np.arange(16)[None, :]) % 6
        idx = np.array(pairs, np.uint8)[pair].reshape(16, 32)
        ref, _ = fr.smfmac_f16_ref(A, idx, B)
        D = run_sp(gf, A, idx, B)[0]
        differ = np.count_nonzero(bits_f32(D) != bits_f32(ref.astype(np.float32)))
        print(f"sparse {name} index pairs: {differ} of 256 elements differ from the "
              "per-element formula")
        assert np.all(np.isfinite(D))


# --- burns -------------------------------------------------------------------------------

ACCS = 8


def f64_burn_model(iters):
    """The burn kernel's data through the pinned maps: lane l holds
    A[l&15][l>>4] = 1 + l%3 and B[l>>4][l&15] = 1 + (l^(l>>3))%3; accumulator n
    of 8 starts at n; lane l stores Σ_n Σ_r acc_n[r], r ↔ D[(l>>4)+4r][l&15]."""
    l = np.arange(64)
    A, B = np.zeros((16, 4), np.int64), np.zeros((4, 16), np.int64)
    A[l & 15, l >> 4] = 1 + l % 3
    B[l >> 4, l & 15] = 1 + (l ^ (l >> 3)) % 3
    assert A.min() >= 1 and B.min() >= 1
    D = A @ B
    lanes = np.array([sum(n + iters * D[(x >> 4) + 4 * r, x & 15]
                          for n in range(ACCS) for r in range(4)) for x in range(64)])
    assert lanes.max() < 2 ** 24
    return lanes.astype(np.float32)


def i8_burn_model(iters):
    """Element j of lane l is 1 + (l+j)%3 in A[l&15][16(l>>4)+j] and
    1 + (l^j)%3 in B[16(l>>4)+j][l&15]; lane l stores the i32 sum
    Σ_n Σ_r acc_n[r], r ↔ D[4(l>>4)+r][l&15]."""
    l, j = np.arange(64)[:, None], np.arange(16)[None, :]
    A, B = np.zeros((16, 64), np.int64), np.zeros((64, 16), np.int64)
    A[l & 15, 16 * (l >> 4) + j] = 1 + (l + j) % 3
    B[16 * (l >> 4) + j, l & 15] = 1 + (l ^ j) % 3
    assert A.min() >= 1 and B.min() >= 1
    D = A @ B
    lanes = [sum(n + iters * D[4 * (x >> 4) + r, x & 15]
                 for n in range(ACCS) for r in range(4)) for x in range(64)]
    return np.array([fr.wrap_i32(int(v)) for v in lanes], np.int32)


@pytest.mark.parametrize("iters", [1, 3])
def test_f64_burn_lanes_match_model(gf, iters):
    r = gf.mfma_f64_burn_run(0, iters, 2)
    assert r["blocks"] == 2 and r["mismatches"] == 0, r
    want = f64_burn_model(iters)
    assert np.unique(want).size > 8                 # the data varies by lane
    assert_bits_equal(np.frombuffer(r["lanes"], np.float32), want, f"iters={iters}")


@pytest.mark.parametrize("iters", [1, 3])
def test_i8_burn_lanes_match_model(gf, iters):
    r = gf.mfma_i8_burn_run(0, iters, 2)
    assert r["blocks"] == 2 and r["mismatches"] == 0, r
    want = i8_burn_model(iters)
    assert np.unique(want).size > 8
    assert_bits_equal(np.frombuffer(r["lanes"], np.int32), want, f"iters={iters}")


@pytest.mark.parametrize("form", ["f64", "i8"])
def test_burn_every_wave_agrees(gf, cus, form):
    r = getattr(gf, f"mfma_{form}_burn_run")(0, 3)
    assert r["blocks"] == 2 * cus
    assert r["mismatches"] == 0, r["mismatches"]


# --- probe -------------------------------------------------------------------------------

FORMS = ("f64", "f16", "i8", "sparse_f16")


@pytest.fixture(scope="module")
def probe_short(gf):
    return gf.mfma_probe_formats(0, 500)


@pytest.fixture(scope="module")
def probe_long(gf):
    return gf.mfma_probe_formats(0, 20000)


def test_probe_formats_healthy(probe_short, probe_long, cus):
    for r in (probe_short, probe_long):
        assert r["blocks"] == 2 * cus
        for form in FORMS:
            assert r[f"{form}_ok"] is True, (form, r)
            assert r[f"{form}_slab_mismatches"] == 0, (form, r)
        for form in ("f64", "i8"):
            assert r[f"{form}_burn_mismatches"] == 0, (form, r)
            assert r[f"{form}_burn_ms"] > 0, (form, r)
        assert r["f64_tflops"] > 0 and r["i8_tops"] > 0, r


def test_burn_time_grows_with_iters(probe_short, probe_long):
    """The timed launch does the work it is credited with: 40 times the
    iterations take longer on the device."""
    for form in ("f64", "i8"):
        short, long_ = probe_short[f"{form}_burn_ms"], probe_long[f"{form}_burn_ms"]
        print(f"{form} burn: {short:.3f} ms at 500 iterations, {long_:.3f} ms at 20000")
        assert long_ > short, (form, short, long_)


def test_probe_rates_above_floors(probe_long):
    from kata_xpu_device_plugin_amd.health import gpuprobe
    r = probe_long
    print(f"f64 {r['f64_tflops']:.1f} TF in {r['f64_burn_ms']:.2f} ms, "
          f"i8 {r['i8_tops']:.0f} TOPS in {r['i8_burn_ms']:.2f} ms")
    assert r["f64_tflops"] >= gpuprobe.F64_TFLOPS_FLOOR_MI355X, r
    assert r["i8_tops"] >= gpuprobe.I8_TOPS_FLOOR_MI355X, r


def test_probe_device_matrix_formats():
    from kata_xpu_device_plugin_amd.health.gpuprobe import probe_device
    rep = probe_device(0, bandwidth_bytes=64 << 20, memtest_bytes=64 << 20,
                       burn_iters=2000, matrix_formats=True)
    assert rep.passed, rep.failures
    assert rep.mfma_f64_ok and rep.mfma_f16_ok and rep.mfma_i8_ok and rep.mfma_sparse_f16_ok
    assert rep.f64_tflops > 0 and rep.i8_tops > 0
    for f in ("mfma_f64_slab_mismatches", "mfma_f16_slab_mismatches",
              "mfma_i8_slab_mismatches", "mfma_sparse_f16_slab_mismatches",
              "f64_burn_mismatches", "i8_burn_mismatches"):
        assert getattr(rep, f) == 0, (f, rep.as_dict())
