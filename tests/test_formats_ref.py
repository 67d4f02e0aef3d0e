"""The references of tests/formats_ref.py checked against what this Python
and numpy provide independently. Needs no GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import formats_ref as fr


def test_f16_decoder_matches_numpy_on_every_code():
    codes = np.arange(65536, dtype=np.uint16)
    want = codes.view(np.float16).astype(np.float64)
    got = fr.f16_decode(codes)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))   # -0 too
    assert nan.sum() == 2 * 1023


def test_f16_bits_round_trip():
    vals = [0.0, -0.0, 1.0, -16.0, 65504.0, -65504.0, 2.0 ** -24, 2.0 ** -14, math.inf]
    bits = fr.f16_bits(vals)
    assert bits.tolist() == [0, 0x8000, 0x3C00, 0xCC00, 0x7BFF, 0xFBFF, 1, 0x0400, 0x7C00]
    assert np.array_equal(bits.view(np.float16).astype(np.float64), np.array(vals))
    with pytest.raises(AssertionError):
        fr.f16_bits([1.0 + 2.0 ** -11])


HAND_FMA = [
    # (a, b, c, fma(a, b, c))
    (3.0, 5.0, 7.0, 22.0),
    # (1+2^-52)^2 - 1 = 2^-51 + 2^-104: unfused rounds the square to 1+2^-51
    (1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, -1.0, 2.0 ** -51 + 2.0 ** -104),
    # the product alone is exact; adding 1 rounds to even (down)
    (2.0 ** -30, 2.0 ** -23, 1.0, 1.0),
    (2.0 ** -30, 3 * 2.0 ** -24, 1.0, 1.0 + 2.0 ** -52),        # above the tie: up
    (2.0 ** -600, 2.0 ** -600, 0.0, 0.0),                       # underflow to +0
    (2.0 ** -537, 2.0 ** -537, 0.0, 2.0 ** -1074),              # smallest subnormal
    (-0.0, 5.0, -0.0, -0.0), (-0.0, 5.0, 0.0, 0.0), (1.0, -1.0, 1.0, 0.0),
    (2.0 ** 600, 2.0 ** 600, 0.0, math.inf), (-2.0 ** 600, 2.0 ** 600, 0.0, -math.inf),
    (math.inf, 1.0, 1.0, math.inf), (1.0, 1.0, -math.inf, -math.inf),
]


@pytest.mark.parametrize("a,b,c,want", HAND_FMA)
def test_f64_fma_hand_cases(a, b, c, want):
    got = fr.fma_exact(a, b, c)
    assert fr.bits_f64(got) == fr.bits_f64(want), (got, want)


def test_f64_fma_special_cases_are_nan():
    for a, b, c in [(math.inf, 0.0, 1.0), (math.inf, 1.0, -math.inf), (math.nan, 1.0, 1.0),
                    (1.0, math.nan, 1.0), (1.0, 1.0, math.nan)]:
        assert math.isnan(fr.fma_exact(a, b, c))


def test_f64_fma_matches_an_independent_fma():
    """Against math.fma where this Python has it (3.13); otherwise on
    operands cut to 26 bits, whose product is exact in a double, so that the
    hardware's a*b+c rounds once, like an fma."""
    def cut26(x):
        m, e = math.frexp(x)
        return math.ldexp(round(math.ldexp(m, 26)), e - 26)

    rng = np.random.default_rng(1)
    fma = getattr(math, "fma", None)
    for _ in range(2000):
        a, b, c = (rng.standard_normal(3) * 2.0 ** rng.integers(-40, 40, 3)).tolist()
        if fma is not None:
            want = fma(a, b, c)
        else:
            a, b = cut26(a), cut26(b)
            want = a * b + c
        assert fr.bits_f64(fr.fma_exact(a, b, c)) == fr.bits_f64(want)


def test_f64_chain_and_exact_sum():
    rng = np.random.default_rng(2)
    A, B, C = rng.standard_normal((16, 4)), rng.standard_normal((4, 16)), \
        rng.standard_normal((16, 16))
    D = fr.mfma_f64_chain(A, B, C)
    total, mag = fr.mfma_f64_exact(A, B, C)
    # the chain's first step is exact-rounded, so it is within 4 roundings
    for i in range(16):
        for j in range(16):
            assert abs(Fraction(float(D[i, j])) - total[i][j]) <= 4 * Fraction(2) ** -53 * mag[i][j]
    # integer data: chain, exact sum and numpy agree exactly
    Ai, Bi = rng.integers(-99, 100, (16, 4)), rng.integers(-99, 100, (4, 16))
    Ci = rng.integers(-99, 100, (16, 16))
    D = fr.mfma_f64_chain(Ai, Bi, Ci)
    assert np.array_equal(D, (Ai @ Bi + Ci).astype(np.float64))
    total, _ = fr.mfma_f64_exact(Ai, Bi, None)
    assert [[int(t) for t in row] for row in total] == (Ai @ Bi).tolist()
    assert np.array_equal(fr.mfma_f64_chain(Ai, Bi), (Ai @ Bi).astype(np.float64))


def test_i8_reference_and_wrap():
    rng = np.random.default_rng(3)
    A = rng.integers(-128, 128, (16, 64)).astype(np.int8)
    B = rng.integers(-128, 128, (64, 16)).astype(np.int8)
    want = A.astype(np.int64) @ B.astype(np.int64)
    assert np.array_equal(fr.mfma_i8_ref(A, B), want.astype(np.int32))
    C = np.full((16, 16), 2 ** 31 - 1, np.int32)
    got = fr.mfma_i8_ref(A, B, C)
    assert np.array_equal(got, ((want + C).astype(np.uint64) & 0xFFFFFFFF)
                          .astype(np.uint32).view(np.int32))
    assert fr.wrap_i32(2 ** 31) == -2 ** 31 and fr.wrap_i32(-2 ** 31 - 1) == 2 ** 31 - 1
    # the extremes: 64 · (-128)² = 2^20
    assert fr.mfma_i8_ref(np.full((16, 64), -128), np.full((64, 16), -128))[0, 0] == 2 ** 20


def test_sparse_reference_matches_dense_expansion():
    rng = np.random.default_rng(4)
    A = fr.f16_bits(rng.integers(-16, 17, (16, 32)))
    B = fr.f16_bits(rng.integers(-16, 17, (64, 16)))
    pair = rng.integers(0, 6, (16, 16))
    idx = np.array(fr.INDEX_PAIRS, np.uint8)[pair].reshape(16, 32)
    assert idx.shape == (16, 32) and np.all(idx[:, 0::2] < idx[:, 1::2])
    D, mag = fr.smfmac_f16_ref(A, idx, B)
    dense = fr.sparse_expand(A, idx)
    assert np.count_nonzero(dense) <= 32 * 16
    assert np.array_equal(D, dense @ fr.f16_decode(B))
    assert np.array_equal(mag, np.abs(dense) @ np.abs(fr.f16_decode(B)))
    # arbitrary (reversed, equal) positions too: the formula is per element
    idx = rng.integers(0, 4, (16, 32)).astype(np.uint8)
    D, _ = fr.smfmac_f16_ref(A, idx, B)
    assert np.array_equal(D, fr.sparse_expand(A, idx) @ fr.f16_decode(B))
    # every position really selects another row of B
    one = fr.f16_bits(np.eye(1, 32, 5).repeat(16, 0))
    for v in range(4):
        D, _ = fr.smfmac_f16_ref(one, np.full((16, 32), v, np.uint8), B)
        assert np.array_equal(D, np.tile(fr.f16_decode(B)[4 * 2 + v], (16, 1)))
