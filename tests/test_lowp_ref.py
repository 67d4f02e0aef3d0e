"""The low-precision decoders of tests/lowp_ref.py against torch's float8
types and the MX specification's e2m1 value list."""
import numpy as np
import pytest

import lowp_ref


def same_values(got, want):
    """Equal including the sign of zero; NaN matches NaN."""
    nan = np.isnan(want)
    return (np.array_equal(np.isnan(got), nan) and
            np.array_equal(got[~nan], want[~nan]) and
            np.array_equal(np.signbit(got[~nan]), np.signbit(want[~nan])))


@pytest.mark.parametrize("fmt,dtype", [("e4m3", "float8_e4m3fn"), ("e5m2", "float8_e5m2")])
def test_fp8_tables_match_torch(fmt, dtype):
    torch = pytest.importorskip("torch")
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    want = codes.view(getattr(torch, dtype)).to(torch.float64).numpy()
    assert same_values(lowp_ref.TABLES[fmt], want)


def test_fp8_special_codes():
    assert np.flatnonzero(np.isnan(lowp_ref.E4M3)).tolist() == [0x7F, 0xFF]
    assert not np.any(np.isinf(lowp_ref.E4M3))
    assert lowp_ref.E4M3[0x7E] == 448.0
    assert np.flatnonzero(np.isinf(lowp_ref.E5M2)).tolist() == [0x7C, 0xFC]
    assert np.flatnonzero(np.isnan(lowp_ref.E5M2)).tolist() == [0x7D, 0x7E, 0x7F,
                                                                0xFD, 0xFE, 0xFF]
    assert lowp_ref.E5M2[0x7B] == 57344.0


def test_e2m1_table():
    mags = [0, .5, 1, 1.5, 2, 3, 4, 6]
    assert lowp_ref.E2M1[:8].tolist() == mags
    assert lowp_ref.E2M1[8:].tolist() == [-m for m in mags]
    assert np.signbit(lowp_ref.E2M1[8])
    with pytest.raises(ValueError):
        lowp_ref.decode_e2m1(16)


def test_e8m0_table():
    assert lowp_ref.E8M0[127] == 1.0
    assert lowp_ref.E8M0[0] == 2.0 ** -127
    assert lowp_ref.E8M0[254] == 2.0 ** 127
    assert np.isnan(lowp_ref.E8M0[255])


def test_code_of_round_trips():
    for fmt in ("e4m3", "e5m2", "e2m1"):
        for c in lowp_ref.finite_codes(fmt):
            v = lowp_ref.TABLES[fmt][c]
            assert lowp_ref.TABLES[fmt][lowp_ref.code_of(v, fmt)] == v
