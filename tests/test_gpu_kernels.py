"""GPU-tier kernel tests: every HIP probe kernel against an independent
reference (tests/refnum.py), at the values and sizes where it can go wrong.

* f32 MFMA tile  — bitwise against an exact k-ordered fmaf chain.
* bf16 MFMA tile — |D − fp64 ref| ≤ 16·2^-23·Σ|a·b| (products exact in f32,
  16 additions of ≤ 1 ulp each in any order); exact cases bitwise.
* burn, LDS, copy, memtest, pointer chase — exact.

Each test is one launch or a handful of launches on tiny buffers.
"""
import numpy as np
import pytest

from refnum import bf16_bits_to_f64, bf16_round_bits, bits_f32, mfma_f32_chain

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def gp():
    from kata_xpu_device_plugin_amd import _gpuprobe
    if _gpuprobe.device_count() == 0:
        pytest.fail("no GPU visible — these tests require a MI355X")
    return _gpuprobe


@pytest.fixture(scope="module")
def cus(gp):
    return gp.device_info(0)["compute_units"]


@pytest.fixture(scope="module")
def grid(cus):
    """Elements covered by one pass of the copy/memtest grid (8×CUs×256)."""
    return 8 * cus * 256


# --- f32 tile ----------------------------------------------------------------

def run_f32(gp, A, B, C=None, blocks=1):
    A = np.ascontiguousarray(A, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    if C is not None:
        C = np.ascontiguousarray(C, np.float32)
    raw = gp.mfma_f32_tile_run(0, A, B, C, blocks)
    return np.frombuffer(raw, np.float32).reshape(blocks, 16, 16)


def assert_bits_equal(got, want, what=""):
    g, w = bits_f32(got).reshape(-1), bits_f32(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (
        f"{what}: {bad.size} of {g.size} elements differ; first: " +
        ", ".join(f"[{i}] got {g[i]:#010x} want {w[i]:#010x}" for i in bad[:6]))


def rand_f32(rng, shape, lo=-20, hi=20):
    """Full-mantissa values: normal × 2^randint(lo, hi)."""
    return (rng.standard_normal(shape) *
            2.0 ** rng.integers(lo, hi + 1, shape)).astype(np.float32)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_f32_tile_random_is_fmaf_chain(gp, seed):
    rng = np.random.default_rng(seed)
    A, B, C = rand_f32(rng, (16, 4)), rand_f32(rng, (4, 16)), rand_f32(rng, (16, 16))
    assert np.all(C != 0)
    assert_bits_equal(run_f32(gp, A, B, C)[0], mfma_f32_chain(A, B, C), f"seed {seed}")


def test_f32_tile_k_order_matters(gp):
    """Products 2^24, 1, -2^24, 1 in k order (row-scaled by 2^(i-8)): the
    k-ordered chain gives 1 (the first +1 is absorbed, the second is not);
    any other order gives 0 or 2."""
    A = np.empty((16, 4), np.float32)
    B = np.empty((4, 16), np.float32)
    scale = 2.0 ** (np.arange(16) - 8)
    A[:, 0], A[:, 1], A[:, 2], A[:, 3] = 4096 * scale, scale, -4096 * scale, scale
    B[0], B[1], B[2], B[3] = 4096, 1, 4096, 1
    ref = mfma_f32_chain(A, B)
    assert np.array_equal(ref, np.repeat(scale[:, None], 16, 1).astype(np.float32))
    assert_bits_equal(run_f32(gp, A, B)[0], ref, "k-order")


def test_f32_tile_subnormals(gp):
    """Subnormal products (rounded at the 2^-149 grid), subnormal A inputs
    and a subnormal C: C/D never flush, and A/B keep denormals in the
    default kernel mode."""
    i = np.arange(16, dtype=np.float64)
    A = np.zeros((16, 4), np.float32)
    B = np.zeros((4, 16), np.float32)
    A[:, 0] = 2.0 ** -80 * (1 + i / 16)
    B[0] = 2.0 ** -60 * (1 + i * 2.0 ** -10)       # product ≈ 2^-140: subnormal
    A[:, 1] = 2.0 ** -140 * (i + 1)                # subnormal input
    B[1] = 2.0 ** (i - 12)
    A[:, 2] = 2.0 ** -75 * (1 + i * 2.0 ** -20)
    B[2] = -(2.0 ** -70) * (1 + i / 32)
    C = ((np.arange(256) + 1) * 2.0 ** -149).astype(np.float32).reshape(16, 16)
    ref = mfma_f32_chain(A, B, C)
    assert np.all(np.abs(ref) < 2.0 ** -126) and np.count_nonzero(ref) > 200
    assert_bits_equal(run_f32(gp, A, B, C)[0], ref, "subnormal")
    # subnormal C alone passes through untouched
    Z = np.zeros((16, 4), np.float32)
    assert_bits_equal(run_f32(gp, Z, Z.reshape(4, 16), C)[0], C, "subnormal C")


@pytest.mark.parametrize("special", [-0.0, np.inf, -np.inf, np.nan])
def test_f32_tile_special_value_stays_in_its_row(gp, special):
    rng = np.random.default_rng(11)
    A, B, C = rand_f32(rng, (16, 4)), rand_f32(rng, (4, 16)), rand_f32(rng, (16, 16))
    row, k = 5, 2
    A[row, k] = special
    D = run_f32(gp, A, B, C)[0]
    ref = mfma_f32_chain(A, B, C)
    others = np.arange(16) != row
    assert_bits_equal(D[others], ref[others], f"{special}: other rows")
    assert np.all(np.isfinite(D[others]))
    if np.isnan(special):
        assert np.all(np.isnan(D[row]))
    elif np.isinf(special):
        assert np.array_equal(D[row], np.float32(special) * np.sign(B[k]))
    else:
        assert_bits_equal(D[row], ref[row], "-0.0 row")


@pytest.mark.parametrize("k0", range(4))
def test_f32_tile_k_slice(gp, k0):
    """Only column k0 of A and row k0 of B are non-zero; every (i, j)
    product is unique and exact, so any operand or output mapping error
    moves a value."""
    A = np.zeros((16, 4), np.float32)
    B = np.zeros((4, 16), np.float32)
    A[:, k0] = 2.0 ** (np.arange(16) - 8)
    B[k0] = 1 + np.arange(16) / 16
    want = np.outer(A[:, k0], B[k0]).astype(np.float32)
    assert np.unique(want).size == 256
    assert_bits_equal(run_f32(gp, A, B)[0], want, f"k0={k0}")


def test_f32_tile_every_cu(gp, cus):
    rng = np.random.default_rng(3)
    A, B, C = rand_f32(rng, (16, 4)), rand_f32(rng, (4, 16)), rand_f32(rng, (16, 16))
    D = run_f32(gp, A, B, C, blocks=2 * cus)
    assert_bits_equal(D[0], mfma_f32_chain(A, B, C), "slab 0")
    bad = [b for b in range(1, 2 * cus) if not np.array_equal(bits_f32(D[b]), bits_f32(D[0]))]
    assert not bad, f"slabs differing from slab 0: {bad[:16]}"


# --- bf16 tile ---------------------------------------------------------------

def run_bf16(gp, A_bits, B_bits, blocks=1):
    raw = gp.mfma_bf16_tile_run(0, np.ascontiguousarray(A_bits, np.uint16),
                                np.ascontiguousarray(B_bits, np.uint16), blocks)
    return np.frombuffer(raw, np.float32).reshape(blocks, 32, 32)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bf16_tile_random_within_derived_bound(gp, seed):
    rng = np.random.default_rng(100 + seed)
    A_bits = bf16_round_bits(rand_f32(rng, (32, 16), -8, 8))
    B_bits = bf16_round_bits(rand_f32(rng, (16, 32), -8, 8))
    A, B = bf16_bits_to_f64(A_bits), bf16_bits_to_f64(B_bits)
    ref, mag = A @ B, np.abs(A) @ np.abs(B)
    D = run_bf16(gp, A_bits, B_bits)[0].astype(np.float64)
    ratio = np.abs(D - ref) / (16 * EPS * mag)
    print(f"bf16 tile seed {seed}: worst error/bound = {ratio.max():.4f}")
    assert np.all(ratio <= 1.0), (ratio.max(), np.argwhere(ratio > 1.0)[:6])


@pytest.mark.parametrize("k0", range(16))
def test_bf16_tile_k_slice(gp, k0):
    """Pins the 8·(l>>5)+j operand map and the (reg&3)+8(reg>>2)+4(l>>5)
    output map: one k at a time, unique exact products."""
    A = np.zeros((32, 16), np.float32)
    B = np.zeros((16, 32), np.float32)
    A[:, k0] = 2.0 ** (np.arange(32) - 16)
    B[k0] = 1 + np.arange(32) / 32
    A_bits, B_bits = bf16_round_bits(A), bf16_round_bits(B)
    assert np.array_equal(bf16_bits_to_f64(A_bits), A)   # exact in bf16
    assert np.array_equal(bf16_bits_to_f64(B_bits), B)
    want = np.outer(A[:, k0], B[k0]).astype(np.float32)
    assert np.unique(want).size == 1024
    assert_bits_equal(run_bf16(gp, A_bits, B_bits)[0], want, f"k0={k0}")


def small_int_bf16(rng):
    """Integer-valued tiles: every product and partial sum is exact in f32,
    so the fp64 product is the bitwise answer under any summation order."""
    A = rng.integers(-8, 9, (32, 16)).astype(np.float32)
    B = rng.integers(-8, 9, (16, 32)).astype(np.float32)
    return A, B, bf16_round_bits(A), bf16_round_bits(B)


def test_bf16_tile_nan_stays_in_its_row(gp):
    A, B, A_bits, B_bits = small_int_bf16(np.random.default_rng(5))
    row = 7
    A_bits[row, 3] = 0x7FC0
    A[row, 3] = 0
    D = run_bf16(gp, A_bits, B_bits)[0]
    want = (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)
    others = np.arange(32) != row
    assert np.all(np.isnan(D[row]))
    assert_bits_equal(D[others], want[others], "rows without NaN")


def test_bf16_tile_every_cu(gp, cus):
    A, B, A_bits, B_bits = small_int_bf16(np.random.default_rng(6))
    D = run_bf16(gp, A_bits, B_bits, blocks=2 * cus)
    want = (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)
    assert_bits_equal(D[0], want, "slab 0")
    bad = [b for b in range(1, 2 * cus) if not np.array_equal(bits_f32(D[b]), bits_f32(D[0]))]
    assert not bad, f"slabs differing from slab 0: {bad[:16]}"


# --- bf16 burn ---------------------------------------------------------------

def burn_model():
    """fp64 model of one burn MFMA: the kernel's a[j], b[j] formulas in f32,
    rounded to bf16, laid out as A[l&31][8(l>>5)+j], B[8(l>>5)+j][l&31];
    returns per-lane Σ_reg (A·B)[row(reg, l>>5)][l&31]."""
    l, j = np.arange(64)[:, None], np.arange(8)[None, :]
    a = np.float32(0.5) + np.float32(0.001) * ((l + j) & 7).astype(np.float32)
    b = np.float32(0.25) + np.float32(0.002) * ((l ^ j) & 7).astype(np.float32)
    assert a.dtype == b.dtype == np.float32
    A = np.zeros((32, 16))
    B = np.zeros((16, 32))
    A[l & 31, 8 * (l >> 5) + j] = bf16_bits_to_f64(bf16_round_bits(a))
    B[8 * (l >> 5) + j, l & 31] = bf16_bits_to_f64(bf16_round_bits(b))
    D = A @ B
    lanes = np.zeros(64)
    for l in range(64):
        for reg in range(16):
            lanes[l] += D[(reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5), l & 31]
    return lanes


@pytest.mark.parametrize("iters", [1, 3])
def test_bf16_burn_lanes_match_model(gp, iters):
    r = gp.mfma_bf16_burn_run(0, iters, 2)
    lanes = np.frombuffer(r["lanes"], np.float32).astype(np.float64)
    want = 4 * iters * burn_model()          # all terms positive: Σ|terms| = want
    ratio = np.abs(lanes - want) / ((16 * iters + 64) * EPS * want)
    print(f"bf16 burn iters={iters}: worst error/bound = {ratio.max():.2e}")
    assert np.all(ratio <= 1.0), (ratio.max(), lanes[:4], want[:4])


def test_bf16_burn_every_wave_agrees(gp, cus):
    r = gp.mfma_bf16_burn_run(0, 3)
    assert r["blocks"] == 2 * cus
    assert r["mismatches"] == 0, r["mismatches"]


# --- LDS burn ----------------------------------------------------------------

@pytest.mark.parametrize("iters", [1, 7, 1822])
def test_lds_burn_sums_exact(gp, cus, iters):
    """Lane t sums slots t + 256m (m = 0..7), whose .x hold their index:
    iters × (8t + 7168), exact in f32 up to iters = 1822."""
    out = np.frombuffer(gp.lds_read_burn_run(0, iters), np.float32).reshape(-1, 256)
    assert out.shape[0] == 4 * cus
    want = (iters * (8 * np.arange(256) + 7168)).astype(np.float32)
    assert want[-1] == iters * 9208 < 2 ** 24
    bad = np.argwhere(out != want[None, :])
    assert bad.size == 0, (len(bad), bad[:8], out[tuple(bad[0])])


# --- copy and memtest --------------------------------------------------------

def sizes(grid):
    return [1, grid - 1, grid, grid + 1, 2 * grid + 3]


def test_memtest_sizes(gp, grid):
    for n in sizes(grid):
        r = gp.memtest(0, 8 * n)
        assert (r["mismatches"], r["bytes"]) == (0, 8 * n), (n, r)
    r = gp.memtest(0, 8 * (grid + 1) + 5)        # floor to whole words
    assert (r["mismatches"], r["bytes"]) == (0, 8 * (grid + 1)), r


def test_copy_check_sizes(gp, grid):
    for n4 in sizes(grid):
        r = gp.hbm_copy_check(0, 16 * n4)
        assert (r["mismatches"], r["bytes"]) == (0, 16 * n4), (n4, r)
    r = gp.hbm_copy_check(0, 16 * (grid + 1) + 13)   # floor to whole float4
    assert (r["mismatches"], r["bytes"]) == (0, 16 * (grid + 1)), r


def test_bandwidth_probe_copy_is_checked(gp, grid):
    for n4 in sizes(grid):
        r = gp.hbm_bandwidth_probe(0, 16 * n4 + 9, 1)
        assert r["copy_mismatches"] == 0, (n4, r)
        assert r["bytes_moved"] == 2 * 16 * n4


@pytest.mark.parametrize("xor", [1, 1 << 63])
def test_memtest_counts_injected_corruption(gp, grid, xor):
    """The probe can fail: each corrupted word is counted exactly once,
    including the first word, the last word and both sides of a grid pass."""
    n = 2 * grid + 3
    offsets = [0, n - 1, grid - 1, grid, n // 2]
    for off in offsets:
        r = gp.memtest(0, 8 * n, corrupt_offsets=[off], corrupt_xor=xor)
        assert r["mismatches"] == 1, (off, r)
    r = gp.memtest(0, 8 * n, corrupt_offsets=offsets, corrupt_xor=xor)
    assert r["mismatches"] == len(offsets), r


@pytest.mark.parametrize("size", ["1", "G", "G+1"])
def test_memtest_last_word_is_checked(gp, grid, size):
    n = {"1": 1, "G": grid, "G+1": grid + 1}[size]
    r = gp.memtest(0, 8 * n, corrupt_offsets=[n - 1])
    assert r["mismatches"] == 1, (n, r)


# --- pointer chase -----------------------------------------------------------

def sattolo_next(n):
    """The probe's chain, rebuilt independently: Sattolo shuffle driven by
    the 64-bit LCG seeded with 0x9E3779B97F4A7C15."""
    mask = (1 << 64) - 1
    perm = list(range(n))
    rng = 0x9E3779B97F4A7C15
    for i in range(n - 1, 0, -1):
        rng = (rng * 6364136223846793005 + 1442695040888963407) & mask
        j = rng % i
        perm[i], perm[j] = perm[j], perm[i]
    nxt = [0] * n
    for i in range(n):
        nxt[perm[i]] = perm[(i + 1) % n]
    return nxt


@pytest.mark.parametrize("steps", [1, 1023, 1024, 5000])
def test_pointer_chase_ends_where_the_host_walk_does(gp, steps):
    n = 1024
    r = gp.hbm_latency_probe(0, 4 * n, steps)
    assert r["final_index"] == r["expected_index"], r
    nxt = sattolo_next(n)
    idx = 0
    for _ in range(steps):
        idx = nxt[idx]
    assert r["expected_index"] == idx, (r, idx)
    if steps % n == 0:
        assert r["expected_index"] == 0     # one full cycle returns to 0
    else:
        assert r["expected_index"] != 0     # …and only a full cycle does
