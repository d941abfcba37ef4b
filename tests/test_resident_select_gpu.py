"""cyto_select and cyto_value_range (csrc/resident.hip) on the GPU against numpy: dst = src[np.ix_(rows, cols)].astype(dst type),
for every source and destination type, with and without row and column lists, in the 16-byte and the one-element forms of the
kernel; the count of values that do not survive the conversion; untouched padding; the refusals; poisoned work buffers; one
table whose element offsets pass 2^31; tables with more rows than the launches have row blocks (4 096 / 256: the stride loops every
real table takes); every workgroup size and a partial last lane in both forms; and each alignment condition of the 16-byte form
broken alone.  Integer data and byte comparisons: nothing has a tolerance."""
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


# ---- the row stride loops, the lane and workgroup edges, the wide form's preconditions --------------------------------------------

PLANTED = {"uint16": [255, 256, 65535, 0],
           "int64": [-1, 255, 256, 65535, 65536, 2**24, 2**24 + 1, 2**53 + 1, -(2**63), 2**63 - 1],
           "float32": [-1, 255, 256, 65535, 65536, 2**24, 2**24 + 2, 0.5, -0.0, np.inf, -np.inf, np.nan],
           "float64": [-1, 255, 256, 65535, 65536, 2**24, 2**24 + 1, 0.5, -0.0, np.inf, -np.inf, np.nan, 2.0**53 + 2, 1e300, 0.1]}


def select_at(src_ptr, shape, ld, src, rows, cols, dst, ld_dst, lead=0):
    """cyto_select into a FILL-ed buffer whose Gs x ld_dst matrix begins `lead` elements in and is followed by 5 more; returns
    (status, the Gs x Cs block, inexact) after asserting that every byte outside the block still holds FILL."""
    Gs = shape[0] if rows is None else len(rows)
    Cs = shape[1] if cols is None else len(cols)
    dt = np.dtype(DST[dst][0])
    n = lead + Gs * ld_dst + 5
    out = _lib.DeviceBuffer.from_numpy(np.full(n * dt.itemsize, FILL, np.uint8))
    bad = ctypes.c_int64(-7)
    try:
        st = _lib.lib().cyto_select(shape[0], shape[1], src_ptr, ld, SRC[src][1], _ptr(rows), Gs, _ptr(cols), Cs, out.ptr + lead * dt.itemsize,
                                    ld_dst, DST[dst][1], ctypes.byref(bad), 0, None)
        raw = out.to_numpy((n * dt.itemsize,), np.uint8)
    finally:
        out.free()
    body = raw.view(dt)[lead:lead + Gs * ld_dst].reshape(Gs, ld_dst)
    mask = np.zeros(n, bool)
    mask[lead:lead + Gs * ld_dst].reshape(Gs, ld_dst)[:, :Cs] = True
    assert (raw[~np.repeat(mask, dt.itemsize)] == FILL).all(), (src, dst, shape, ld_dst, lead, "bytes outside the block written")
    return st, np.ascontiguousarray(body[:, :Cs]), bad.value


def check_select_at(src_ptr, host, shape, ld, src, rows, cols, dst, ld_dst, lead=0):
    view = host[:shape[0], :shape[1]][np.ix_(np.arange(shape[0]) if rows is None else rows, np.arange(shape[1]) if cols is None else cols)]
    st, block, bad = select_at(src_ptr, shape, ld, src, rows, cols, dst, ld_dst, lead)
    tag = (src, dst, shape, ld, ld_dst, lead, None if rows is None else len(rows), None if cols is None else len(cols))
    assert st == 0, tag
    want, ok, defined = expect(view, dst)
    assert bad == int(np.count_nonzero(~ok)), (tag, bad)
    wrong = (block.view(np.uint8).reshape(block.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,))).any(-1) & defined
    assert not wrong.any(), (tag, f"{wrong.sum()} elements differ; rows {np.flatnonzero(wrong.any(1))[:8]}, columns {np.flatnonzero(wrong.any(0))[:8]}")
    return block, defined


def expect_range(view):
    """What cyto_value_range reports for the view, from numpy."""
    if view.dtype.kind in "iu":
        return dict(lo=float(int(view.min())), hi=float(int(view.max())), ilo=int(view.min()), ihi=int(view.max()), non_integral=0, non_finite=0,
                    not_f32_exact=int(np.count_nonzero(~survives(view, "float32"))))
    v = view.astype(np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(v)
        return dict(lo=float(np.nanmin(v)), hi=float(np.nanmax(v)), ilo=0, ihi=0, non_finite=int(np.count_nonzero(~fin)),
                    non_integral=int(np.count_nonzero(fin & (np.trunc(v) != v))),
                    not_f32_exact=int(np.count_nonzero(~np.isnan(v) & (v.astype(np.float32).astype(np.float64) != v))))


TALL_G, TALL_C, TALL_LD = 4100, 9, 16
TALL_ROWS = (0, 255, 256, 4095, 4096, 4099)


def _tall(name):
    """4 100 x 9 with ld = 16: every element of the table differs from every other (9 i + j + 300), so a row that is skipped, read
    twice or written to another place shows; rows 0, 255, 256, 4095, 4096 and 4099 hold the planted values of the type.  The
    table's minimum, its maximum and (float64) a value that float32 does not hold lie in rows 4096 and 4099 only."""
    dt = SRC[name][0]
    a = np.full((TALL_G, TALL_LD), 77 if name == "uint16" else np.nan, dt)
    a[:, :TALL_C] = (9 * np.arange(TALL_G)[:, None] + np.arange(TALL_C)[None, :] + 300).astype(dt)
    planted = [v for v in PLANTED[name] if v == v and abs(v) != np.inf and v not in (0, 65535, 1e300, -1)]
    for k, r in enumerate(TALL_ROWS):
        for j in range(0, TALL_C, 2):
            a[r, j] = planted[(3 * k + j) % len(planted)]
    if name == "uint16":
        a[4096, 4], a[4099, 7] = 0, 65535
    else:
        a[4096, 4], a[4099, 7], a[4099, 3], a[4096, 1] = -1, 1e300, 0.1, 2.0**53 + 2
    return np.ascontiguousarray(a)


@pytest.fixture(scope="module")
def tall_sources(hip_lib):
    host = {name: _tall(name) for name in ("uint16", "float64")}
    bufs = {name: _lib.DeviceBuffer.from_numpy(host[name]) for name in host}
    yield host, bufs
    for b in bufs.values():
        b.free()


def _tall_row_lists():
    rng = np.random.default_rng(21)
    full = rng.permutation(TALL_G).astype(np.int64)
    full[rng.integers(0, TALL_G, 40)] = rng.integers(0, TALL_G, 40)              # a permutation with repeats
    full[[0, 4095, 4096, 4099]] = (4099, 0, 4095, 4096)                           # the planted rows at both ends of the grid and behind it
    short = np.ascontiguousarray(full[:4097])
    short[4096] = 4099                                                           # position 4096: the one row of the second trip of the loop
    return {"no list": None, "4100 positions": full, "4097 positions": short}


@pytest.mark.gpu
@pytest.mark.parametrize("src", ["uint16", "float64"])
def test_select_walks_every_row_beyond_the_grid(src, tall_sources):
    """MAX_ROW_BLOCKS = 4096: with more rows than that -- every real table -- a workgroup walks its rows in a stride loop."""
    host, bufs = tall_sources
    cols = np.array([8, 0, 3, 3, 7, 1, 8, 2, 4, 5, 6], np.int64)
    for rname, rows in _tall_row_lists().items():
        Gs = TALL_G if rows is None else len(rows)
        assert Gs > 4096
        for dst in (("uint16", "int64", "uint8") if src == "uint16" else ("float64", "float32", "uint16")):
            check_select_at(bufs[src].ptr, host[src], (TALL_G, TALL_C), TALL_LD, src, rows, None, dst, 16)      # the 16-byte form
            check_select_at(bufs[src].ptr, host[src], (TALL_G, TALL_C), TALL_LD, src, rows, None, dst, TALL_C + 2)
            check_select_at(bufs[src].ptr, host[src], (TALL_G, TALL_C), TALL_LD, src, rows, cols, dst, len(cols) + 2)


@pytest.mark.gpu
@pytest.mark.parametrize("src", ["uint16", "float64"])
def test_value_range_walks_every_row_beyond_the_grid(src, tall_sources):
    """RANGE_ROW_BLOCKS = 256.  The view's minimum and maximum (and, float64, a value float32 does not hold) lie in rows >= 4096 of
    the table, at list positions the first trip of the loop does not reach wherever the list is longer than the grid."""
    host, bufs = tall_sources
    rng = np.random.default_rng(22)
    low = rng.permutation(4096)[:300].astype(np.int64)
    lists = {256: np.r_[low[:254], 4096, 4099], 257: np.r_[low[:255], 4096, 4099], 4100: None,
             "4100 listed": np.r_[rng.permutation(4096), 4096, 4097, 4098, 4099].astype(np.int64)}
    cols = np.array([7, 4, 3, 1, 0, 7], np.int64)
    table = host[src][:, :TALL_C]
    for name, rows in lists.items():
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        assert rows is None or len(rows) == (name if isinstance(name, int) else 4100)
        for c in (None, cols):
            r_, c_ = (np.arange(TALL_G) if rows is None else rows), (np.arange(TALL_C) if c is None else c)
            want = expect_range(table[np.ix_(r_, c_)])
            inside = table[np.ix_(r_[r_ < 4096], c_)]
            assert inside.min() > want["lo"] and inside.max() < want["hi"]           # (the extremes are in rows >= 4096 only)
            assert src == "uint16" or want["not_f32_exact"] > expect_range(inside)["not_f32_exact"]
            assert value_range(bufs[src].ptr, (TALL_G, TALL_C), TALL_LD, src, rows, c) == want, (src, name, c is not None)


EDGE_G, EDGE_C, EDGE_LD = 3, 2056, 2064          # (2064 elements: a multiple of 16 bytes in every source type)
EDGE_CS = sorted(set([1, 63, 64, 65, 128, 129, 256, 257] + list(range(2, 18)) + [127, 130, 131, 255, 258, 259, 511, 512, 513, 515, 519, 1023,
                                                                                   1024, 1025, 1027, 1031, 2049, 2051, 2055]))


def _edge(name, ld=EDGE_LD):
    dt = SRC[name][0]
    rng = np.random.default_rng(30 + sorted(SRC).index(name))
    a = rng.poisson(3.0, (EDGE_G, ld)).astype(dt)
    planted = PLANTED[name]
    where = rng.permutation(EDGE_G * EDGE_C)[:40 * len(planted)]
    for k, w in enumerate(where):
        a[w // EDGE_C, w % EDGE_C] = planted[k % len(planted)]
    a[:, EDGE_C:] = 77 if name in ("uint16", "int64") else np.nan
    return np.ascontiguousarray(a)


@pytest.mark.gpu
@pytest.mark.parametrize("src", sorted(SRC))
def test_lane_and_workgroup_edges(src, hip_lib):
    """Workgroups of 64, 128 and 256 lanes (lanes <= 64, <= 128, more), in the one-element form (a lane per column: Cs around 64, 128,
    256) and in the 16-byte form (a lane per VEC = 16 / element size columns: Cs around 64 VEC and 128 VEC), whose last lane is
    partial wherever Cs is no multiple of VEC -- 8 k + 1 ... 8 k + 7 for uint16, 4 k + 1 ... 3 for float32, odd for the 8-byte types."""
    host = _edge(src)
    buf = _lib.DeviceBuffer.from_numpy(host)
    rng = np.random.default_rng(31)
    dsts = {"uint16": ("uint16", "int64"), "int64": ("int64", "uint8"), "float32": ("float32", "float64"), "float64": ("float64", "uint16")}[src]
    try:
        assert buf.ptr % 16 == 0
        for Cs in EDGE_CS:
            cols = np.ascontiguousarray(np.r_[rng.integers(0, EDGE_C, Cs - 1), EDGE_C - 1][::-1].astype(np.int64))
            for dst in dsts:
                # without a list the view is the first Cs columns of a table of that width: ld_dst a multiple of 16 bytes (the 16-byte
                # form where Cs >= VEC), and not
                check_select_at(buf.ptr, host, (EDGE_G, Cs), EDGE_LD, src, None, None, dst, Cs + 16 + (-Cs) % 16)
                check_select_at(buf.ptr, host, (EDGE_G, Cs), EDGE_LD, src, None, None, dst, Cs + 1 + Cs % 2)
                check_select_at(buf.ptr, host, (EDGE_G, EDGE_C), EDGE_LD, src, None, cols, dst, Cs + 3)
            view = host[:, :Cs]
            assert value_range(buf.ptr, (EDGE_G, Cs), EDGE_LD, src, None, None) == expect_range(view), (src, Cs)
            assert value_range(buf.ptr, (EDGE_G, EDGE_C), EDGE_LD, src, None, cols) == expect_range(host[:, :EDGE_C][:, cols]), (src, Cs)
    finally:
        buf.free()


@pytest.mark.gpu
@pytest.mark.parametrize("src", sorted(SRC))
def test_each_precondition_of_the_16_byte_form_alone(src, hip_lib):
    """launch_select takes the 16-byte form where the source base, ld_src, the destination base and ld_dst are all aligned for it.  Each
    of the four is broken alone: the same bits, and nothing outside the block is written."""
    item = np.dtype(SRC[src][0]).itemsize
    Cs = 1031
    host = _edge(src)
    odd = _edge(src, 2057)
    odd[:, :EDGE_C] = host[:, :EDGE_C]
    assert (EDGE_LD * item) % 16 == 0 and (2057 * item) % 16 != 0
    buf, obuf = _lib.DeviceBuffer.from_numpy(host), _lib.DeviceBuffer.from_numpy(odd)
    try:
        for dst in sorted(DST):
            aligned, defined = check_select_at(buf.ptr, host, (EDGE_G, Cs), EDGE_LD, src, None, None, dst, 1040)
            variants = {"ld_src": check_select_at(obuf.ptr, odd, (EDGE_G, Cs), 2057, src, None, None, dst, 1040),
                        "destination base": check_select_at(buf.ptr, host, (EDGE_G, Cs), EDGE_LD, src, None, None, dst, 1040, lead=1),
                        "ld_dst": check_select_at(buf.ptr, host, (EDGE_G, Cs), EDGE_LD, src, None, None, dst, 1033)}
            for name, (block, _) in variants.items():
                assert np.array_equal(block.view(np.uint8)[np.repeat(defined, block.itemsize, 1)],
                                      aligned.view(np.uint8)[np.repeat(defined, block.itemsize, 1)]), (src, dst, name)
            # the source base one element in: the view is then the columns 1 ... Cs of the table
            shifted, d2 = check_select_at(buf.ptr + item, host[:, 1:], (EDGE_G, Cs - 1), EDGE_LD, src, None, None, dst, 1040)
            m = np.repeat(defined[:, 1:] & d2, shifted.itemsize, 1)
            assert np.array_equal(shifted.view(np.uint8)[m], np.ascontiguousarray(aligned[:, 1:]).view(np.uint8)[m]), (src, dst, "source base")
    finally:
        buf.free()
        obuf.free()
