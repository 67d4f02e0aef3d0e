"""Independent references for the FP64 / FP16 / INT8 / 2:4-sparse matrix-core
kernels of probes/xpu_probe_formats.hip. Nothing here shares code with the
.hip file: f64 is exact rational arithmetic rounded once per step, f16 is
decoded from its bits by hand, i8 is Python integers, sparse is the formula.
"""
import math
from fractions import Fraction

import numpy as np


# --- f64 ---------------------------------------------------------------------

def fma_exact(a: float, b: float, c: float) -> float:
    """IEEE-754 f64 fused multiply-add: a*b+c evaluated exactly as a Fraction
    and rounded once (float(Fraction) rounds to nearest even, subnormals
    included)."""
    a, b, c = float(a), float(b), float(c)
    if math.isnan(a) or math.isnan(b) or math.isnan(c):
        return math.nan
    if math.isinf(a) or math.isinf(b):
        if a == 0.0 or b == 0.0:
            return math.nan
        p = math.copysign(math.inf, a) * math.copysign(1.0, b)
        if math.isinf(c) and c != p:
            return math.nan
        return p
    if math.isinf(c):
        return c
    q = Fraction(a) * Fraction(b) + Fraction(c)
    if q == 0:
        # exact zero: the sign survives only when both addends are zeros of
        # the same sign; otherwise round-to-nearest gives +0
        psign = math.copysign(1.0, a) * math.copysign(1.0, b)
        if (a == 0.0 or b == 0.0) and c == 0.0 and psign == math.copysign(1.0, c):
            return math.copysign(0.0, c)
        return 0.0
    try:
        return float(q)
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def _f64_tiles(A, B, C):
    A = np.asarray(A, np.float64).reshape(16, 4)
    B = np.asarray(B, np.float64).reshape(4, 16)
    C = np.zeros((16, 16)) if C is None else np.asarray(C, np.float64).reshape(16, 16)
    return A, B, C


def mfma_f64_chain(A, B, C=None) -> np.ndarray:
    """16×16 = A(16×4)·B(4×16)+C as the k-ordered chain
    fma(a3,b3, fma(a2,b2, fma(a1,b1, fma(a0,b0, C)))), each step exact and
    rounded once."""
    A, B, C = _f64_tiles(A, B, C)
    D = np.empty((16, 16), np.float64)
    for i in range(16):
        for j in range(16):
            acc = float(C[i, j])
            for k in range(4):
                acc = fma_exact(A[i, k], B[k, j], acc)
            D[i, j] = acc
    return D


def mfma_f64_exact(A, B, C=None):
    """The exact sums C + Σ a·b and the magnitudes |C| + Σ|a·b| as 16×16
    nested lists of Fractions (finite inputs only)."""
    A, B, C = _f64_tiles(A, B, C)
    total = [[Fraction(float(C[i, j])) +
              sum(Fraction(float(A[i, k])) * Fraction(float(B[k, j])) for k in range(4))
              for j in range(16)] for i in range(16)]
    mag = [[abs(Fraction(float(C[i, j]))) +
            sum(abs(Fraction(float(A[i, k])) * Fraction(float(B[k, j]))) for k in range(4))
            for j in range(16)] for i in range(16)]
    return total, mag


def bits_f64(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# --- f16 ---------------------------------------------------------------------

def f16_decode_one(code: int) -> float:
    """IEEE binary16 bits → value, by hand: 1 sign, 5 exponent (bias 15),
    10 mantissa bits; exponent 0 is subnormal, 31 is inf / NaN."""
    sign = -1.0 if code & 0x8000 else 1.0
    e, m = (code >> 10) & 31, code & 0x3FF
    if e == 31:
        return sign * math.inf if m == 0 else math.nan
    if e == 0:
        return sign * m * 2.0 ** -24
    return sign * (1024 + m) * 2.0 ** (e - 25)


_F16_TABLE = np.array([f16_decode_one(c) for c in range(65536)], np.float64)


def f16_decode(bits) -> np.ndarray:
    return _F16_TABLE[np.asarray(bits, np.uint16).astype(np.int64)]


def f16_bits(values) -> np.ndarray:
    """Values exactly representable in f16 → their bit patterns, found in the
    decode table (no numpy.float16 on the way); -0.0 keeps its sign."""
    v = np.asarray(values, np.float64)
    out = np.empty(v.shape, np.uint16)
    pos = _F16_TABLE[:0x7C01]                       # +0 .. +inf, ascending
    for idx in np.ndindex(v.shape):
        x = float(v[idx])
        if math.isnan(x):
            out[idx] = 0x7E00
            continue
        i = int(np.searchsorted(pos, abs(x)))
        assert i < len(pos) and pos[i] == abs(x), f"{x!r} is not an f16 value"
        out[idx] = i | (0x8000 if math.copysign(1.0, x) < 0 else 0)
    return out


def mfma_f16_ref(A_bits, B_bits):
    """fp64 product and Σ|a·b| of a 32×16 by 16×32 tile of f16 bit patterns."""
    a = f16_decode(np.asarray(A_bits).reshape(32, 16))
    b = f16_decode(np.asarray(B_bits).reshape(16, 32))
    return a @ b, np.abs(a) @ np.abs(b)


# --- i8 ----------------------------------------------------------------------

def wrap_i32(v: int) -> int:
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def mfma_i8_ref(A, B, C=None) -> np.ndarray:
    """16×16 int32 = A(16×64 int8)·B(64×16 int8)+C in Python integers, reduced
    mod 2^32 once at the end."""
    A = np.asarray(A).reshape(16, 64)
    B = np.asarray(B).reshape(64, 16)
    D = np.empty((16, 16), np.int32)
    for i in range(16):
        for j in range(16):
            s = 0 if C is None else int(np.asarray(C).reshape(16, 16)[i, j])
            for k in range(64):
                s += int(A[i, k]) * int(B[k, j])
            D[i, j] = wrap_i32(s)
    return D


# --- 2:4 sparse f16 ------------------------------------------------------------

def smfmac_f16_ref(A_bits, A_idx, B_bits):
    """D[i][j] = Σ_e A[i][e] · B[4(e>>1) + idx[i][e]][j] in fp64, and the sum of
    the magnitudes. A_bits is the 16×32 kept half, B_bits the dense 64×16."""
    a = f16_decode(np.asarray(A_bits).reshape(16, 32))
    idx = np.asarray(A_idx).reshape(16, 32).astype(np.int64)
    b = f16_decode(np.asarray(B_bits).reshape(64, 16))
    assert idx.min() >= 0 and idx.max() <= 3
    D = np.zeros((16, 16))
    mag = np.zeros((16, 16))
    for i in range(16):
        for e in range(32):
            row = b[4 * (e >> 1) + idx[i, e]]
            D[i] += a[i, e] * row
            mag[i] += abs(a[i, e]) * np.abs(row)
    return D, mag


def sparse_expand(A_bits, A_idx) -> np.ndarray:
    """The dense 16×64 A (as values) that the kept half and its positions
    stand for; two kept elements at one position add up."""
    a = f16_decode(np.asarray(A_bits).reshape(16, 32))
    idx = np.asarray(A_idx).reshape(16, 32).astype(np.int64)
    dense = np.zeros((16, 64))
    for i in range(16):
        for e in range(32):
            dense[i, 4 * (e >> 1) + idx[i, e]] += a[i, e]
    return dense


INDEX_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
