"""Independent high-precision references for the HIP probe kernels.

Nothing here shares code with probes/xpu_probe.hip: the f32 reference is
exact rational arithmetic rounded once, the bf16 reference is fp64.
"""
import math
from fractions import Fraction

import numpy as np

_TWO = Fraction(2)


def round_to_f32(q: Fraction) -> float:
    """Round an exact non-zero rational once to f32: ties-to-even, gradual
    underflow (ulp never below 2^-149), overflow to inf."""
    sign = -1.0 if q < 0 else 1.0
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if _TWO ** e > q:
        e -= 1
    elif _TWO ** (e + 1) <= q:
        e += 1
    assert _TWO ** e <= q < _TWO ** (e + 1)
    ulp = _TWO ** (max(e, -126) - 23)
    n = q / ulp
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    val = fl * ulp
    if val >= _TWO ** 128:
        return sign * math.inf
    return sign * float(val)  # ≤ 24 significant bits: exact in a double


def fmaf_exact(a, b, c) -> np.float32:
    """IEEE-754 f32 fused multiply-add of f32 values: a*b+c evaluated
    exactly, rounded once."""
    a, b, c = float(a), float(b), float(c)
    if math.isnan(a) or math.isnan(b) or math.isnan(c):
        return np.float32(math.nan)
    if math.isinf(a) or math.isinf(b):
        if a == 0.0 or b == 0.0:
            return np.float32(math.nan)
        p = math.copysign(math.inf, a) * math.copysign(1.0, b)
        if math.isinf(c) and c != p:
            return np.float32(math.nan)
        return np.float32(p)
    if math.isinf(c):
        return np.float32(c)
    q = Fraction(a) * Fraction(b) + Fraction(c)
    if q == 0:
        # exact zero: the sign survives only when both addends are zeros
        # of the same sign; otherwise round-to-nearest gives +0
        psign = math.copysign(1.0, a) * math.copysign(1.0, b)
        if (a == 0.0 or b == 0.0) and c == 0.0 and psign == math.copysign(1.0, c):
            return np.float32(math.copysign(0.0, c))
        return np.float32(0.0)
    return np.float32(round_to_f32(q))


def mfma_f32_chain(A, B, C=None) -> np.ndarray:
    """16×16 = A(16×4)·B(4×16)+C as the k-ordered fmaf chain
    fma(a3,b3, fma(a2,b2, fma(a1,b1, fma(a0,b0, C))))."""
    A = np.asarray(A, np.float32).reshape(16, 4)
    B = np.asarray(B, np.float32).reshape(4, 16)
    C = np.zeros((16, 16), np.float32) if C is None else \
        np.asarray(C, np.float32).reshape(16, 16)
    D = np.empty((16, 16), np.float32)
    for i in range(16):
        for j in range(16):
            acc = C[i, j]
            for k in range(4):
                acc = fmaf_exact(A[i, k], B[k, j], acc)
            D[i, j] = acc
    return D


def bf16_round_bits(x) -> np.ndarray:
    """f32 → bf16 bit patterns, round-to-nearest-even; NaN → quiet NaN."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    r[nan] = ((u[nan] >> 16) | 0x0040).astype(np.uint16)
    return r


def bf16_bits_to_f64(bits) -> np.ndarray:
    bits = np.ascontiguousarray(bits, np.uint16)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bits_f32(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
