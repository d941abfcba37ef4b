"""The layout builder of the device-input tests (tests/_layouts.py) on the CPU: the data lands where it claims, everything else is
poison, and the base alignment is the one the layout's name promises."""
import numpy as np
import pytest

import _layouts as LY

DTYPES = (np.float32, np.float64, np.uint16, np.uint8)
SHAPES = ((1, 1), (2, 2), (5, 5), (33, 4), (7, 63), (3, 301), (4, 1000), (3, 1001), (6, 260))


def _matrix(rows, n, dtype):
    # every element distinct from every poison: small positive counts
    return (1 + np.arange(rows * n).reshape(rows, n) % 200).astype(dtype)


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LY.LAYOUTS)
def test_data_lands_where_claimed_and_the_rest_is_poison(layout, dtype, W):
    for rows, n in SHAPES:
        x = _matrix(rows, n, dtype)
        for poison in LY.POISONS:
            buf, lead, ld = LY.build(x, layout, W, poison)
            p = LY.poison_value(dtype, poison)
            assert buf.dtype == x.dtype and buf.ndim == 1 and ld >= n and len(buf) == lead + rows * ld + LY.TAIL
            # the data: element (i, j) at lead + i * ld + j, read back both through extract and by plain index arithmetic
            assert np.array_equal(LY.extract(buf, lead, ld, rows, n), x)
            i, j = np.divmod(np.arange(rows * n), n)
            assert np.array_equal(buf[lead + i * ld + j], x.ravel())
            # everything else: the poison's very bits (NaN included)
            mask = LY.data_mask(rows, n, lead, ld)
            assert mask.sum() == rows * n
            rest = LY.bits(buf[~mask])
            assert len(rest) == len(buf) - rows * n and (rest == LY.bits(np.array([p], dtype))[0]).all()
            assert len(rest) >= LY.TAIL and not mask[:lead].any() and not mask[lead + rows * ld:].any()
            if np.dtype(dtype).kind == "f" and np.isnan(poison):
                assert np.isnan(buf[~mask]).all()


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 255, 256, 301, 302, 1000, 1001, 1028])
def test_pitch_and_base_are_as_named(n, W):
    pad = LY.round_up(n, W)
    got = {name: LY.pitch_and_lead(n, name, W) for name in LY.LAYOUTS}
    assert got["tight"] == (n, 0)
    assert got["padded"] == (pad, 0) and pad % W == 0 and 0 <= pad - n < W
    ld, lead = got["wide"]
    assert lead == 0 and ld % W == 0 and ld == pad + 2 * W            # aligned, and wider than any padded width of n
    ld, lead = got["double"]
    assert lead == 0 and ld % W == 0 and 2 * n <= ld < 2 * n + W
    ld, lead = got["odd_pitch"]
    assert lead == 0 and ld % W != 0 and n < ld <= n + 2
    assert got["offset_base"] == (pad, 1) and got["quad_offset_base"] == (pad, W)
    for dtype in DTYPES:
        e = np.dtype(dtype).itemsize
        for name in ("tight", "padded", "wide", "double", "odd_pitch"):
            assert LY.base_alignment(got[name][1], e) == LY.ALLOC_ALIGN
        assert LY.base_alignment(got["offset_base"][1], e) == e           # aligned to the element and to nothing more
        assert LY.base_alignment(got["quad_offset_base"][1], e) == W * e  # aligned to the quad and to nothing more
    # one quad of four: 16 bytes for float32, but only 8 for uint16 and 4 for uint8
    assert [LY.base_alignment(4, np.dtype(d).itemsize) for d in DTYPES] == [16, 32, 8, 4]


def test_integer_poison_is_the_maximum_and_skipped_rows_are_poison():
    assert LY.poison_value(np.uint8, -1e30) == 255 and LY.poison_value(np.uint16, float("nan")) == 65535
    assert LY.poison_value(np.float32, -1e30) == np.float32(-1e30) and np.isneginf(LY.poison_value(np.float64, float("-inf")))
    x = _matrix(6, 10, np.float32)
    buf, lead, ld = LY.build(x, "wide", 4, float("nan"), skip_rows=[1, 4])
    body = buf[lead:lead + 6 * ld].reshape(6, ld)
    assert np.isnan(body[[1, 4]]).all() and np.array_equal(body[[0, 2, 3, 5], :10], x[[0, 2, 3, 5]])
    mask = LY.data_mask(6, 10, lead, ld, skip_rows=[1, 4])
    assert mask.sum() == 40 and np.isnan(buf[~mask]).all() and not np.isnan(buf[mask]).any()
    with pytest.raises(ValueError):
        LY.pitch_and_lead(8, "diagonal")
