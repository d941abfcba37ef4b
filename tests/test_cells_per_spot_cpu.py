"""cyto_normalized_colsums: the argument checks need no device (status codes only)."""
import ctypes

import numpy as np


def _matrix(_lib, data, ld, code, on_device=0):
    m = _lib.Matrix()
    m.data, m.ld, m.is_f64, m.on_device = data, ld, code, on_device
    return m


def test_normalized_colsums_argument_validation_needs_no_device():
    from cytospace_amd import _lib
    L = _lib.lib()
    BAD = 1   # CYTO_ERR_BAD_ARG
    x = np.zeros((4, 4), np.float64)
    sums = np.zeros(4, np.float64)
    ok = _matrix(_lib, x.ctypes.data, 4, _lib.CYTO_DTYPE_F64)
    for call, extra in ((L.cyto_normalized_colsums, ()), (L.cyto_normalized_colsums_timed, (None,))):
        assert call(0, 4, ctypes.byref(ok), sums.ctypes.data, 0, None, *extra) == BAD                 # G <= 0
        assert call(4, 0, ctypes.byref(ok), sums.ctypes.data, 0, None, *extra) == BAD                 # C <= 0
        assert call(-1, 4, ctypes.byref(ok), sums.ctypes.data, 0, None, *extra) == BAD
        assert call(4, 4, None, sums.ctypes.data, 0, None, *extra) == BAD                             # no matrix
        assert call(4, 4, ctypes.byref(ok), None, 0, None, *extra) == BAD                             # no output
        null = _matrix(_lib, None, 4, _lib.CYTO_DTYPE_F64)
        assert call(4, 4, ctypes.byref(null), sums.ctypes.data, 0, None, *extra) == BAD               # no data
        short = _matrix(_lib, x.ctypes.data, 3, _lib.CYTO_DTYPE_F64)
        assert call(4, 4, ctypes.byref(short), sums.ctypes.data, 0, None, *extra) == BAD              # ld < C
        for code in (-1, _lib.CYTO_DTYPE_I32, _lib.CYTO_DTYPE_I64, 6):                               # a dtype outside the four
            other = _matrix(_lib, x.ctypes.data, 4, code)
            assert call(4, 4, ctypes.byref(other), sums.ctypes.data, 0, None, *extra) == BAD
        for dev in (0, 1):                                                                           # (the same for a device matrix)
            short = _matrix(_lib, x.ctypes.data, 3, _lib.CYTO_DTYPE_U8, dev)
            assert call(4, 4, ctypes.byref(short), sums.ctypes.data, 0, None, *extra) == BAD
    assert not sums.any()


def test_normalized_column_sums_refuses_what_is_not_a_matrix():
    import pytest
    from cytospace_amd import common
    with pytest.raises(ValueError):
        common.normalized_column_sums(np.zeros(5))
    with pytest.raises(ValueError):
        common.normalized_column_sums(np.zeros((0, 5)))
    with pytest.raises(ValueError):
        common.normalized_column_sums(np.zeros((5, 0), np.int64))
