"""Cells per spot: the column sums of the normalised ST table on the device (cyto_normalized_colsums, common.normalized_column_sums,
cytospace.estimate_cell_number_RNA_reads).  The oracle everywhere is what the function replaced,

    want = common.normalize_data(x64).sum(axis=0, dtype=float)

and every comparison is np.array_equal: the same float64 bits, never a tolerance.  (One shape needs a second oracle: a table of one
column, which numpy adds pairwise; see test_sums_equal_numpys_sum_of_normalize_data.)"""
import ctypes
import functools
import os

import numpy as np
import pytest

from cytospace_amd import _lib
from cytospace_amd import common as gcommon
from cytospace_amd import cytospace as gcyto
from cytospace_amd.resident import DeviceFrame

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

DTYPES = {np.dtype(np.float32): _lib.CYTO_DTYPE_F32, np.dtype(np.float64): _lib.CYTO_DTYPE_F64,
          np.dtype(np.uint16): _lib.CYTO_DTYPE_U16, np.dtype(np.uint8): _lib.CYTO_DTYPE_U8}

GS = (1, 2, 63, 64, 255, 256, 257, 513, 1030)        # cross the 256-gene partial block, normalize_write's 64 and the kernel's tiles
CS = (1, 3, 4, 63, 64, 65, 256, 260, 515)            # cross the quad, the wave and the block widths
# every G and every C twice, the corners, a long single column, and two wide tables: at 2 x 256 blocks of 32 and of 64 columns the
# launcher leaves the 16-column kernel (on a device with fewer CUs, sooner)
SHAPES = sorted({(G, CS[i]) for i, G in enumerate(GS)} | {(G, CS[(i + 4) % 9]) for i, G in enumerate(GS)} |
                {(1, 1), (1030, 515), (257, 3), (2, 260), (1030, 1)}) + [(67, 32 * 512 + 5), (67, 64 * 512 + 5)]


@functools.lru_cache(maxsize=None)
def _counts(G, C):
    c = np.random.default_rng(1000 * G + C).poisson(5.0, (G, C))
    assert c.max() < 256
    c.setflags(write=False)
    return c


def _want(x64):
    return gcommon.normalize_data(np.ascontiguousarray(x64, dtype=np.float64)).sum(axis=0, dtype=float)


@functools.lru_cache(maxsize=None)
def _want_counts(G, C):
    w = _want(_counts(G, C))
    w.setflags(write=False)
    return w


def _abi(G, C, data, ld, dtype, on_device):
    """cyto_normalized_colsums itself, in the dtype given (the Python layer would narrow it)."""
    m = _lib.Matrix()
    m.data, m.ld, m.is_f64, m.on_device = data, ld, DTYPES[np.dtype(dtype)], on_device
    out = np.full(C, -7.0)
    _lib.check(_lib.lib().cyto_normalized_colsums(G, C, ctypes.byref(m), out.ctypes.data, 0, None))
    return out


def _host(x):
    x = np.ascontiguousarray(x)
    return _abi(x.shape[0], x.shape[1], x.ctypes.data, x.shape[1], x.dtype, 0)


def _rows_in_order(x64):
    """The rows of normalize_data's matrix added one after the other on the host: numpy's own order for two columns or more."""
    y = gcommon.normalize_data(np.ascontiguousarray(x64, dtype=np.float64))
    s = y[0].copy()
    for g in range(1, len(y)):
        s += y[g]
    return s


@pytest.mark.parametrize("G,C", SHAPES)
def test_sums_equal_numpys_sum_of_normalize_data(G, C):
    counts, want = _counts(G, C), _want_counts(G, C)
    # One column is a contiguous vector to numpy, which adds it pairwise (measured: (256, 1) differs from the row loop in the last
    # bit): the Python entry point gives numpy's bits there too, the C entry point the rows in order, as its header says.
    want_abi = want if C > 1 else _rows_in_order(counts)
    for dt in DTYPES:
        got = _host(counts.astype(dt))
        assert np.array_equal(got, want_abi), (str(dt), int((got != want_abi).sum()), float(np.abs(got - want_abi).max()))
    # the Python entry point: int64 counts go up as uint8, the same numbers
    assert np.array_equal(gcommon.normalized_column_sums(counts), want)
    assert gcommon.normalized_column_sums(counts).dtype == np.float64


def test_the_order_of_the_adds_is_pinned():
    # numpy adds the rows of a C-contiguous matrix in order; the pairwise sum of each column (the transposed copy's reduce) has other
    # bits somewhere, so a kernel that reassociates cannot pass the test above
    G, C = 1030, 65
    y = gcommon.normalize_data(_counts(G, C).astype(np.float64))
    want = _want_counts(G, C)
    assert np.array_equal(_rows_in_order(_counts(G, C)), want)
    pairwise = np.add.reduce(np.ascontiguousarray(y.T), axis=1)
    assert (pairwise != want).any()
    assert np.array_equal(_host(_counts(G, C).astype(np.uint8)), want)


def _special(dtype):
    G, C = 70, 13                       # (two tiles of the 16-column kernel, the second partial)
    rng = np.random.default_rng(3)
    x = rng.poisson(3.0, (G, C)).astype(np.float64)
    x[:, 0] = 0.0                                                   # all zero: 0 * inf -> NaN -> 0
    x[5, 1] = np.nan
    x[69, 1] = np.nan
    x[7, 2] = np.inf
    x[8, 3] = -np.inf
    x[9, 4], x[10, 4], x[66, 4] = np.nan, np.inf, -np.inf
    x[:, 5] = -x[:, 5] - 1.0                                        # negative entries, a negative sum
    x[::3, 6] *= -1.0                                               # negative entries, a positive sum
    x[:, 7] = np.where(np.arange(G) % 2 == 0, 4.0, -4.0)            # the sum cancels to 0
    x[:, 8] = 1e300 if dtype == np.float64 else 1e38
    x[3, 9] = 1e300 if dtype == np.float64 else 3e38
    x[:, 10] = 0.0
    x[69, 10] = 2.0                                                 # the only count in the last row
    x[:, 11] = rng.random(G) * 1e-3                                 # fractions
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x.astype(dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_special_values(dtype):
    x = _special(dtype)
    assert x[:, 5].sum() < 0 and x[:, 7].sum() == 0
    want = _want(x.astype(np.float64))
    got = _host(x)
    assert np.array_equal(got, want, equal_nan=True), (got, want)
    assert np.array_equal(gcommon.normalized_column_sums(x), want, equal_nan=True)


def _device_layout(x, ld, lead):
    """x in a device buffer of 0xFF bytes with `lead` elements before the first and ld elements per row: (buffer, pointer)."""
    G, C = x.shape
    host = np.full((lead + G * ld + 3) * x.itemsize, 0xFF, np.uint8)
    rows = host[lead * x.itemsize:(lead + G * ld) * x.itemsize].view(x.dtype).reshape(G, ld)
    rows[:, :C] = x
    buf = _lib.DeviceBuffer.from_numpy(host)
    assert buf.ptr % 16 == 0
    return buf, buf.ptr + lead * x.itemsize


@pytest.mark.parametrize("dtype", list(DTYPES), ids=str)
@pytest.mark.parametrize("G,C", [(257, 260), (130, 67)])
def test_device_inputs_give_the_host_bits(G, C, dtype):
    x = _counts(G, C).astype(dtype)
    want = _want_counts(G, C)
    assert np.array_equal(_host(x), want)
    for ld in (C, C + 1, C + 5):
        for lead in (0, 1, 16 // x.itemsize):       # a 16-byte aligned base, one element past it, the next aligned one
            buf, ptr = _device_layout(x, ld, lead)
            try:
                got = _abi(G, C, ptr, ld, dtype, 1)
                assert np.array_equal(got, want), (ld, lead)
            finally:
                buf.free()


def _gv7():
    import pandas as pd
    d = np.load(os.path.join(GOLD, "gv7_upstream.npz"))
    st = d["st_counts"]
    st_df = pd.DataFrame(st, index=[f"g{i}" for i in range(st.shape[0])], columns=[f"s{i}" for i in range(st.shape[1])])
    return d, st_df


@pytest.mark.parametrize("kind", [np.int64, np.float64])
def test_estimate_on_a_device_frame_gives_the_golden_cells_per_spot(kind):
    d, st_df = _gv7()
    frame = DeviceFrame.from_frame(st_df.astype(kind))
    try:
        for mean in (5, 20):
            got = gcyto.estimate_cell_number_RNA_reads(frame, mean)
            assert np.array_equal(got, d[f"cells_per_spot_mean{mean}"])
            assert np.array_equal(gcyto.estimate_cell_number_RNA_reads(st_df.astype(kind), mean), d[f"cells_per_spot_mean{mean}"])
        assert frame.fetches == 0
    finally:
        frame.close()


def test_estimate_on_a_view_of_a_device_frame():
    d, st_df = _gv7()
    G, S = st_df.shape
    rng = np.random.default_rng(7)
    rows = rng.permutation(G)[:max(2, (3 * G) // 4)]
    cols = rng.permutation(S)[:max(2, (2 * S) // 3)]
    frame = DeviceFrame.from_frame(st_df.astype(np.int64))
    try:
        view = frame.take(rows=rows, cols=cols)
        sub = st_df.iloc[rows, cols]
        want = _want(sub.values.astype(float))
        assert np.array_equal(gcommon.normalized_column_sums(view), want)
        assert np.array_equal(gcommon.normalized_column_sums(sub.values), want)
        for mean in (5, 20):
            assert np.array_equal(gcyto.estimate_cell_number_RNA_reads(view, mean), gcyto.estimate_cell_number_RNA_reads(sub, mean))
        assert frame.fetches == 0
        # one spot: numpy adds a single column pairwise, and so does this (through numpy, with a fetch of the column)
        one = st_df.iloc[:, [3]]
        assert np.array_equal(gcommon.normalized_column_sums(frame.take(cols=[3])), _want(one.values.astype(float)))
        assert np.array_equal(gcommon.normalized_column_sums(one.values), _want(one.values.astype(float)))
    finally:
        frame.close()


def test_the_kernel_time_is_reported():
    counts = _counts(257, 260)
    got, ms = gcommon.normalized_column_sums(counts, return_kernel_ms=True)
    assert np.array_equal(got, _want_counts(257, 260)) and 0.0 < ms < 1000.0
