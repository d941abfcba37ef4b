"""cyto_select and cyto_value_range (csrc/resident.hip) on the GPU against numpy: dst = src[np.ix_(rows, cols)].astype(dst type),
for every source and destination type, with and without row and column lists, in the 16-byte and the one-element forms of the
kernel; the count of values that do not survive the conversion; untouched padding; the refusals; poisoned work buffers; and one
table whose element offsets pass 2^31.  Integer data and byte comparisons: nothing has a tolerance."""
import ctypes
import warnings

import numpy as np
import pytest

from cytospace_amd import _lib

SRC = {"int64": (np.int64, _lib.CYTO_DTYPE_I64), "float64": (np.float64, _lib.CYTO_DTYPE_F64),
       "uint16": (np.uint16, _lib.CYTO_DTYPE_U16), "float32": (np.float32, _lib.CYTO_DTYPE_F32)}
DST = dict(SRC, uint8=(np.uint8, _lib.CYTO_DTYPE_U8))
G, C, LD = 67, 131, 136
FILL = 0xA5
_RNG = np.random.default_rng(20)
ROWS = _RNG.permutation(G)[:41].astype(np.int64)
ROWS[7] = ROWS[30]                                            # out of order, one repeat
COLS = np.ascontiguousarray(np.r_[_RNG.integers(0, C, 199), C - 1][::-1].astype(np.int64))     # 200 positions with repeats, reversed
COLS[:2] = (C - 1, 0)


def _source(name):
    """G x LD of the type: counts below 200 (they survive every conversion) with the planted values of the issue scattered in,
    in the first C columns; the padding columns hold what no view may read."""
    rng = np.random.default_rng(sorted(SRC).index(name))
    a = rng.poisson(3.0, (G, LD)).astype(np.int64)
    if name == "uint16":
        planted = [255, 256, 65535, 0]
    elif name == "int64":
        planted = [-1, 255, 256, 65535, 65536, 2**24, 2**24 + 1, 2**53 + 1, -(2**63), 2**63 - 1]
    else:
        planted = [-1, 255, 256, 65535, 65536, 2**24, 2**24 + 1, 0.5, -0.0, np.nan, np.inf, -np.inf] + ([2.0**53 + 2, 1e300, 0.1]
                                                                                                     if name == "float64" else [])
    a = a.astype(SRC[name][0])
    where = rng.permutation(G * C)[:3 * len(planted)]
    for k, w in enumerate(where):
        a[w // C, w % C] = planted[k % len(planted)]
    a[0, 0], a[G - 1, C - 1] = planted[0], planted[1]          # the corners
    a[:, C:] = 77 if name in ("uint16", "int64") else np.nan
    return np.ascontiguousarray(a)


HOST = {name: _source(name) for name in SRC}


@pytest.fixture(scope="module")
def device_sources(hip_lib):
    bufs = {name: _lib.DeviceBuffer.from_numpy(HOST[name]) for name in SRC}
    yield bufs
    for b in bufs.values():
        b.free()


def _ptr(a):
    return None if a is None else a.ctypes.data


def select(src_ptr, shape, ld, src, rows, cols, dst, ld_dst, fill=FILL):
    """cyto_select into a pre-filled Gs x ld_dst buffer; returns (status, the whole buffer on the host, inexact)."""
    Gs = shape[0] if rows is None else len(rows)
    Cs = shape[1] if cols is None else len(cols)
    host = np.full(max(Gs, 1) * ld_dst * np.dtype(DST[dst][0]).itemsize, fill, np.uint8)
    out = _lib.DeviceBuffer.from_numpy(host)
    bad = ctypes.c_int64(-7)
    try:
        st = _lib.lib().cyto_select(shape[0], shape[1], src_ptr, ld, SRC[src][1], _ptr(rows), Gs, _ptr(cols), Cs, out.ptr, ld_dst,
                                    DST[dst][1], ctypes.byref(bad), 0, None)
        got = out.to_numpy((max(Gs, 1), ld_dst), DST[dst][0])
    finally:
        out.free()
    return st, got, bad.value


def survives(v, dst):
    ok = np.empty(v.size, np.int8)
    v = np.ascontiguousarray(v)
    _lib.check(_lib.lib().cyto_select_check(v.ctypes.data, SRC[v.dtype.name][1], v.size, DST[dst][1], ok.ctypes.data))
    return ok.astype(bool).reshape(v.shape)                   # (pinned against numpy's round trip in tests/test_resident_cpu.py)


def expect(view, dst):
    """(the converted view where numpy defines it, the mask of the elements that survive)."""
    ok = survives(view, dst)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if np.dtype(DST[dst][0]).kind == "f":
            return view.astype(DST[dst][0]), ok, np.ones(view.shape, bool)      # (the rounded value is defined for every element)
        safe = np.where(ok, view, 0)
        return safe.astype(DST[dst][0]), ok, ok


def check_select(src_ptr, host, shape, ld, src, rows, cols, dst, ld_dst):
    view = host[:shape[0], :shape[1]][np.ix_(np.arange(shape[0]) if rows is None else rows, np.arange(shape[1]) if cols is None else cols)]
    st, got, bad = select(src_ptr, shape, ld, src, rows, cols, dst, ld_dst)
    assert st == 0
    want, ok, defined = expect(view, dst)
    assert bad == int(np.count_nonzero(~ok)), (src, dst, bad)
    Cs = view.shape[1]
    block = got[:, :Cs]
    assert np.array_equal(block[defined].view(np.uint8), want[defined].view(np.uint8)), (src, dst)     # bits: -0.0 and NaN too
    pad = np.ascontiguousarray(got[:, Cs:]).view(np.uint8)
    assert (pad == FILL).all(), (src, dst, "padding written")
    return bad


VIEWS = [(None, None), (ROWS, None), (None, COLS), (ROWS, COLS)]


@pytest.mark.gpu
@pytest.mark.parametrize("dst", sorted(DST))
@pytest.mark.parametrize("src", sorted(SRC))
def test_select_equals_numpy(src, dst, device_sources):
    total_bad = 0
    for rows, cols in VIEWS:
        Cs = C if cols is None else len(cols)
        for ld_dst in (Cs + 13 + (-(Cs + 13)) % 16, Cs + 2):     # rows of the destination aligned to 16 bytes, and not
            total_bad += check_select(device_sources[src].ptr, HOST[src], (G, C), LD, src, rows, cols, dst, ld_dst)
    if (src, dst) in (("int64", "uint8"), ("float64", "uint16"), ("float32", "int64"), ("float64", "float32"), ("uint16", "uint8")):
        assert total_bad > 0                                   # (the planted values are there)


@pytest.mark.gpu
@pytest.mark.parametrize("src", sorted(SRC))
def test_select_from_an_unaligned_base_and_one_by_one(src, device_sources):
    """One element into the buffer the rows are no longer 16-byte aligned (the one-element form of the kernel), C - 1 columns; and
    the 1 x 1 view at the last element."""
    item = np.dtype(SRC[src][0]).itemsize
    for dst in ("uint16", "float64"):
        check_select(device_sources[src].ptr + item, HOST[src][:, 1:], (G, C - 1), LD, src, None, None, dst, C + 15)
        check_select(device_sources[src].ptr, HOST[src], (G, C), LD, src, np.array([G - 1], np.int64), np.array([C - 1], np.int64), dst, 1)
    one = np.ascontiguousarray(HOST[src][:1, :1])
    buf = _lib.DeviceBuffer.from_numpy(one)
    try:
        check_select(buf.ptr, one, (1, 1), 1, src, None, None, "float64", 1)
    finally:
        buf.free()


@pytest.mark.gpu
def test_empty_extents_and_refusals_leave_the_destination_alone(device_sources):
    p = device_sources["int64"].ptr
    none = np.zeros(0, np.int64)
    for rows, cols in ((none, None), (None, none), (none, none)):
        st, got, bad = select(p, (G, C), LD, "int64", rows, cols, "uint16", C + 1)
        assert st == 0 and bad == 0 and (got.view(np.uint8) == FILL).all()
    L = _lib.lib()
    out = _lib.DeviceBuffer.from_numpy(np.full(G * LD, FILL, np.uint8).repeat(8))
    bad = ctypes.c_int64()
    r1, c1 = np.array([0, G], np.int64), np.array([-1], np.int64)
    ok_r, ok_c = np.array([1, 0], np.int64), np.array([2], np.int64)
    I64, U8, I32 = _lib.CYTO_DTYPE_I64, _lib.CYTO_DTYPE_U8, _lib.CYTO_DTYPE_I32
    calls = {
        "row out of range": (G, C, p, LD, I64, _ptr(r1), 2, None, C, out.ptr, LD, I64),
        "column out of range": (G, C, p, LD, I64, None, G, _ptr(c1), 1, out.ptr, LD, I64),
        "source dtype": (G, C, p, LD, U8, None, G, None, C, out.ptr, LD, I64),
        "destination dtype": (G, C, p, LD, I64, None, G, None, C, out.ptr, LD, I32),
        "ld_src < C": (G, C, p, C - 1, I64, None, G, None, C, out.ptr, LD, I64),
        "ld_dst < Cs": (G, C, p, LD, I64, None, G, None, C, out.ptr, C - 1, I64),
        "null source": (G, C, None, LD, I64, None, G, None, C, out.ptr, LD, I64),
        "null destination": (G, C, p, LD, I64, _ptr(ok_r), 2, _ptr(ok_c), 1, None, LD, I64),
        "no rows but Gs != G": (G, C, p, LD, I64, None, 2, None, C, out.ptr, LD, I64),
        "negative extent": (G, C, p, LD, I64, _ptr(ok_r), -1, None, C, out.ptr, LD, I64),
    }
    try:
        for name, a in calls.items():
            assert L.cyto_select(*a, ctypes.byref(bad), 0, None) == 1, name
            assert L.cyto_select(*a, ctypes.byref(bad), 99, None) == 1, name       # (refused before the device is looked at)
        assert L.cyto_select(G, C, p, LD, I64, None, G, None, C, out.ptr, LD, I64, None, 0, None) == 1      # no `inexact`
        lo, hi = ctypes.c_double(), ctypes.c_double()
        n = [ctypes.c_int64() for _ in range(5)]
        for name in ("row out of range", "column out of range", "source dtype", "ld_src < C", "null source", "no rows but Gs != G"):
            assert L.cyto_value_range(*calls[name][:9], ctypes.byref(lo), ctypes.byref(hi), *[ctypes.byref(x) for x in n], 99, None) == 1, name
        assert (out.to_numpy((G * LD * 8,), np.uint8) == FILL).all()
    finally:
        out.free()


def value_range(src_ptr, shape, ld, src, rows, cols):
    Gs = shape[0] if rows is None else len(rows)
    Cs = shape[1] if cols is None else len(cols)
    lo, hi = ctypes.c_double(), ctypes.c_double()
    ilo, ihi, nint, nfin, n32 = (ctypes.c_int64() for _ in range(5))
    _lib.check(_lib.lib().cyto_value_range(shape[0], shape[1], src_ptr, ld, SRC[src][1], _ptr(rows), Gs, _ptr(cols), Cs, ctypes.byref(lo),
                                           ctypes.byref(hi), ctypes.byref(ilo), ctypes.byref(ihi), ctypes.byref(nint), ctypes.byref(nfin),
                                           ctypes.byref(n32), 0, None))
    return dict(lo=lo.value, hi=hi.value, ilo=ilo.value, ihi=ihi.value, non_integral=nint.value, non_finite=nfin.value,
                not_f32_exact=n32.value)


@pytest.mark.gpu
@pytest.mark.parametrize("src", sorted(SRC))
def test_value_range_equals_numpy(src, device_sources):
    for rows, cols in VIEWS + [(np.array([3], np.int64), np.array([5], np.int64))]:
        view = HOST[src][:, :C][np.ix_(np.arange(G) if rows is None else rows, np.arange(C) if cols is None else cols)]
        got = value_range(device_sources[src].ptr, (G, C), LD, src, rows, cols)
        if view.dtype.kind in "iu":
            assert (got["ilo"], got["ihi"]) == (int(view.min()), int(view.max()))
            assert (got["lo"], got["hi"]) == (float(int(view.min())), float(int(view.max())))
            assert got["non_integral"] == 0 and got["non_finite"] == 0
            assert got["not_f32_exact"] == int(np.count_nonzero(~survives(view, "float32")))
        else:
            v = view.astype(np.float64)
            with np.errstate(all="ignore"):
                assert (got["lo"], got["hi"]) == (float(np.nanmin(v)), float(np.nanmax(v)))
                fin = np.isfinite(v)
                assert got["non_finite"] == int(np.count_nonzero(~fin))
                assert got["non_integral"] == int(np.count_nonzero(fin & (np.trunc(v) != v)))
                assert got["not_f32_exact"] == int(np.count_nonzero(~np.isnan(v) & (v.astype(np.float32).astype(np.float64) != v)))
    empty = value_range(device_sources[src].ptr, (G, C), LD, src, np.zeros(0, np.int64), None)
    assert (empty["lo"], empty["hi"], empty["non_finite"], empty["not_f32_exact"]) == (np.inf, -np.inf, 0, 0)


@pytest.mark.gpu
def test_poisoned_work_buffers_change_nothing(device_sources):
    _lib.cache_poison(0xA5)
    try:
        for src, dst in (("int64", "uint8"), ("float64", "float32"), ("uint16", "int64"), ("float32", "uint16")):
            check_select(device_sources[src].ptr, HOST[src], (G, C), LD, src, ROWS, COLS, dst, len(COLS) + 3)
            check_select(device_sources[src].ptr, HOST[src], (G, C), LD, src, None, None, dst, C + 13)
            clean = value_range(device_sources[src].ptr, (G, C), LD, src, ROWS, COLS)
            _lib.cache_poison(None)
            assert clean == value_range(device_sources[src].ptr, (G, C), LD, src, ROWS, COLS)
            _lib.cache_poison(0xA5)
    finally:
        _lib.cache_poison(None)


@pytest.mark.gpu
def test_offsets_beyond_two_to_the_31(hip_lib):
    """A uint16 table of 33 000 x 66 000 (4.36 GB), zero-filled on the device, with a handful of values planted by small copies in
    rows whose element offset exceeds 2^31 (and whose byte offset exceeds 2^32); those rows are selected, with and without a column
    list.  A 32-bit offset anywhere would read the zeros of a low row."""
    from _hiprt import runtime
    BG, BC = 33000, 66000
    rt = runtime()
    rt.hipMemset.argtypes, rt.hipMemset.restype = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t], ctypes.c_int
    buf = _lib.DeviceBuffer(BG * BC * 2)
    try:
        assert rt.hipMemset(buf.ptr, 0, BG * BC * 2) == 0
        rows = np.array([BG - 1, 32540, 32768, 32540], np.int64)
        assert (rows * BC > 2**31).all() and (rows * BC * 2 > 2**32).all()
        cols = np.array([BC - 1, 0, 40001, 40000, 7, 7], np.int64)
        want = np.zeros((len(rows), BC), np.uint16)
        for k, r in enumerate(rows[:3]):
            for j, c in enumerate(cols[:5]):
                v = np.array([1000 * (k + 1) + j + 1], np.uint16)
                _lib.check(hip_lib.cyto_memcpy_h2d(buf.ptr + (int(r) * BC + int(c)) * 2, v.ctypes.data, 2, 0))
                want[k, c] = v[0]
        want[3] = want[1]
        for dst in ("uint16", "int64"):
            st, got, bad = select(buf.ptr, (BG, BC), BC, "uint16", rows, None, dst, BC)
            assert st == 0 and bad == 0 and np.array_equal(got, want.astype(DST[dst][0]))
            st, got, bad = select(buf.ptr, (BG, BC), BC, "uint16", rows, cols, dst, len(cols) + 2)
            assert st == 0 and bad == 0 and np.array_equal(got[:, :len(cols)], want[:, cols].astype(DST[dst][0]))
        r = value_range(buf.ptr, (BG, BC), BC, "uint16", rows, None)
        assert (r["ilo"], r["ihi"]) == (0, int(want.max()))
    finally:
        buf.free()
