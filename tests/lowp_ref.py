"""Low-precision number formats for the FP8 / MX kernel tests, written from
the OCP format definitions (OFP8 and Microscaling v1.0): code → float64.

    e4m3 (fn)  1-4-3, bias 7; no inf; S.1111.111 (0x7F / 0xFF) is NaN
    e5m2       1-5-2, bias 15; IEEE-style inf (0x7C / 0xFC) and NaNs
    e2m1       1-2-1, bias 1; every code finite
    E8M0       unsigned exponent, bias 127; 0xFF is NaN
"""
import numpy as np


def _decode_minifloat(code, ebits, mbits, bias):
    sign = -1.0 if (code >> (ebits + mbits)) & 1 else 1.0
    e = (code >> mbits) & ((1 << ebits) - 1)
    m = code & ((1 << mbits) - 1)
    if e == 0:
        return sign * m * 2.0 ** (1 - bias - mbits)
    return sign * (1 + m * 2.0 ** -mbits) * 2.0 ** (e - bias)


def decode_e4m3(code):
    if code & 0x7F == 0x7F:
        return float("nan")
    return _decode_minifloat(code, 4, 3, 7)


def decode_e5m2(code):
    e, m = (code >> 2) & 31, code & 3
    if e == 31:
        sign = -1.0 if code & 0x80 else 1.0
        return sign * float("inf") if m == 0 else float("nan")
    return _decode_minifloat(code, 5, 2, 15)


def decode_e2m1(code):
    if not 0 <= code < 16:
        raise ValueError(code)
    return _decode_minifloat(code, 2, 1, 1)


def decode_e8m0(code):
    return float("nan") if code == 0xFF else 2.0 ** (code - 127)


E4M3 = np.array([decode_e4m3(c) for c in range(256)])
E5M2 = np.array([decode_e5m2(c) for c in range(256)])
E2M1 = np.array([decode_e2m1(c) for c in range(16)])
E8M0 = np.array([decode_e8m0(c) for c in range(256)])
TABLES = {"e4m3": E4M3, "e5m2": E5M2, "e2m1": E2M1}


def decode(codes, fmt):
    """uint8 codes → float64 values."""
    return TABLES[fmt][np.asarray(codes, np.int64)]


def finite_codes(fmt):
    t = TABLES[fmt]
    return np.flatnonzero(np.isfinite(t)).astype(np.uint8)


def code_of(value, fmt):
    """The (positive-zero-preferring) code of an exactly representable value."""
    t = TABLES[fmt]
    hit = np.flatnonzero(t == value)
    if hit.size == 0:
        raise ValueError(f"{value} is not an {fmt} value")
    return int(hit[0])


def mx_ref(A_codes, B_codes, A_scales, B_scales, a_fmt, b_fmt):
    """fp64 D[i][j] = Σ_b 2^(sa[i][b]-127)·2^(sb[b][j]-127)·Σ_{k∈b} a·b and the
    same with absolute values (the magnitude the error bounds scale with)."""
    A, B = decode(A_codes, a_fmt), decode(B_codes, b_fmt)
    SA, SB = E8M0[np.asarray(A_scales, np.int64)], E8M0[np.asarray(B_scales, np.int64)]
    As = A * np.repeat(SA, 32, axis=1)
    Bs = B * np.repeat(SB, 32, axis=0)
    return As @ Bs, np.abs(As) @ np.abs(Bs)
