"""Expression tables that stay on the GPU from the reader to the solver.

A DeviceFrame is what a pandas DataFrame of one dtype is to the host path: a genes x cells table with an `index` and `columns`
-- but its values live in HBM (a parsed table's own buffer, or an upload), its labels on the host, and selecting rows or columns
(`take`) only composes position lists.  The stages of cytospace.main_cytospace(resident=True) hand such frames to each other; a
stage that needs the values in another shape asks for them with `materialize` (one device-to-device gather: cyto_select), a stage
that needs them on the host with `to_frame` (counted in `fetches`).  There is no host fallback inside this module: a table it does
not take (mixed int64 / float64 columns, duplicate column labels, another dtype) stays a DataFrame at the caller.
"""
import ctypes

import numpy as np

from . import _lib

# CYTO_DTYPE_* <-> numpy: what a frame can hold (the sources of cyto_select) and what it can be materialised to
_SRC = {np.dtype(np.int64): _lib.CYTO_DTYPE_I64, np.dtype(np.float64): _lib.CYTO_DTYPE_F64,
        np.dtype(np.uint16): _lib.CYTO_DTYPE_U16, np.dtype(np.float32): _lib.CYTO_DTYPE_F32}
_DST = dict(_SRC)
_DST[np.dtype(np.uint8)] = _lib.CYTO_DTYPE_U8

# main_cytospace(resident=True) writes this per run: {"scRNA": report, "ST": report, "fallbacks": [(stage, reason), ...]} with a
# report {"source": "table" (parsed on the device) / "upload" (from_frame) / "host" (it stayed a DataFrame), "fetches": downloads
# of the values, "materialized": gathers on the device}
last_run = {}


def record_fallback(stage, reason):
    """A stage of a resident run went through the host (or a refusal was taken): noted in last_run["fallbacks"]."""
    last_run.setdefault("fallbacks", []).append((stage, reason))


def is_frame(x):
    return isinstance(x, DeviceFrame)


def narrowest_dtype(kind, lo, hi, non_integral, not_f32_exact):
    """The dtype cytospace._counts_matrix chooses for a matrix of dtype `kind` (anything np.dtype takes) from what
    cyto_value_range reports of it: float32 / uint8 / uint16 stay; integers become uint8 / uint16 when lo >= 0 and hi fits, float32
    when max(-lo, hi) < 2^24, else float64 (an empty matrix, lo > hi: float32); float64 becomes float32 when every value survives
    the cast (not_f32_exact == 0; NaN counts as surviving), else stays.  non_integral takes no part: _counts_matrix never makes
    integers of a float matrix."""
    kind = np.dtype(kind)
    if kind in (np.dtype(np.float32), np.dtype(np.uint8), np.dtype(np.uint16)):
        return kind
    if kind.kind in "iub":
        if lo > hi:
            return np.dtype(np.float32)
        lo, hi = int(lo), int(hi)
        if lo >= 0 and hi < (1 << 8):
            return np.dtype(np.uint8)
        if lo >= 0 and hi < (1 << 16):
            return np.dtype(np.uint16)
        if max(-lo, hi) < (1 << 24):
            return np.dtype(np.float32)
        return np.dtype(np.float64)
    return np.dtype(np.float32) if not_f32_exact == 0 else np.dtype(np.float64)


def compose(outer, inner, n):
    """Positions `inner` (into a view of n entries whose own positions into the buffer are `outer`; None: the identity) as
    positions into the buffer.  Negative positions count from the end, like iloc's; IndexError outside [-n, n)."""
    if inner is None:
        return outer
    inner = np.asarray(inner)
    if inner.dtype == bool:
        if inner.shape != (n,):
            raise IndexError("boolean index of the wrong length")
        inner = np.flatnonzero(inner)
    inner = np.ascontiguousarray(inner, dtype=np.int64).reshape(-1)
    if inner.size and (inner.min() < -n or inner.max() >= n):
        raise IndexError("positional indexers are out-of-bounds")
    inner = np.where(inner < 0, inner + n, inner)
    return np.ascontiguousarray(inner if outer is None else outer[inner])


class _Table:
    """Owner of a parsed table (cyto_table handle): its values are borrowed until free()."""

    def __init__(self, handle, device_id):
        self.handle, self.device_id = handle, device_id
        p, ld = ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(_lib.lib().cyto_table_values(handle, ctypes.byref(p), ctypes.byref(ld)))
        self.ptr, self.ld = p.value, ld.value

    def free(self):
        if self.handle is not None:
            _lib.lib().cyto_table_free(self.handle)
            self.handle = self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceFrame:
    """A genes x cells table of one dtype in HBM with its labels on the host; a lazy view (optional row and column positions)
    into a buffer it shares with the frames it was taken from."""

    def __init__(self, owner, shape, ld, dtype, index, columns, rows=None, cols=None, device_id=0, stats=None, source="upload"):
        import pandas as pd
        self._owner, self._shape, self._ld = owner, (int(shape[0]), int(shape[1])), int(ld)
        self.dtype = np.dtype(dtype)
        self.code = _SRC[self.dtype] if self.dtype in _SRC else _DST[self.dtype]
        self._rows, self._cols = rows, cols
        self.device_id = device_id
        self.stats = stats if stats is not None else {"source": source, "fetches": 0, "materialized": 0}
        self._index, self._columns = pd.Index(index), pd.Index(columns)
        if (len(self._index), len(self._columns)) != self.shape:
            raise ValueError("labels do not match the view")

    # ---- labels and shape (host only)
    @property
    def shape(self):
        return (self._shape[0] if self._rows is None else len(self._rows), self._shape[1] if self._cols is None else len(self._cols))

    @property
    def index(self):
        return self._index

    @index.setter
    def index(self, labels):
        import pandas as pd
        labels = pd.Index(labels)
        if len(labels) != self.shape[0]:
            raise ValueError(f"Length mismatch: Expected axis has {self.shape[0]} elements, new values have {len(labels)} elements")
        self._index = labels

    @property
    def columns(self):
        return self._columns

    @columns.setter
    def columns(self, labels):
        import pandas as pd
        labels = pd.Index(labels)
        if len(labels) != self.shape[1]:
            raise ValueError(f"Length mismatch: Expected axis has {self.shape[1]} elements, new values have {len(labels)} elements")
        self._columns = labels

    @property
    def fetches(self):
        return self.stats["fetches"]

    @property
    def materialized(self):
        return self.stats["materialized"]

    @property
    def source(self):
        return self.stats["source"]

    @property
    def ptr(self):
        p = self._owner.ptr
        if not p:
            raise RuntimeError("the frame's buffer was freed")
        return p

    @property
    def ld(self):
        return self._ld

    @property
    def buffer_shape(self):
        """(rows, columns) of the buffer the view looks into."""
        return self._shape

    @property
    def positions(self):
        """(rows, cols): the view's positions into its buffer (None: all, in order)."""
        return self._rows, self._cols

    def _view_args(self):
        r, c = self._rows, self._cols
        G, C = self.shape
        return (self._shape[0], self._shape[1], self.ptr, self._ld, self.code, None if r is None else r.ctypes.data, G,
                None if c is None else c.ctypes.data, C)

    # ---- views
    def take(self, rows=None, cols=None):
        """The frame of these row and column POSITIONS of this one (None: all; repeats allowed, negative positions from the end):
        iloc[rows, cols] on labels and positions alone -- nothing is copied, the buffer is shared."""
        G, C = self.shape
        r = compose(self._rows, rows, G)
        c = compose(self._cols, cols, C)
        index = self._index if rows is None else self._index[compose(None, rows, G)]
        columns = self._columns if cols is None else self._columns[compose(None, cols, C)]
        return DeviceFrame(self._owner, self._shape, self._ld, self.dtype, index, columns, r, c, self.device_id, self.stats)

    def take_labels(self, index=None, columns=None):
        """take() by labels, for unique labels: KeyError if one is missing."""
        rows = cols = None
        if index is not None:
            rows = self._index.get_indexer(index)
            if (rows < 0).any():
                raise KeyError("row labels not found")
        if columns is not None:
            cols = self._columns.get_indexer(columns)
            if (cols < 0).any():
                raise KeyError("column labels not found")
        return self.take(rows, cols)

    # ---- device work
    def _select(self, dtype, allow_inexact=False):
        dtype = self.dtype if dtype is None else np.dtype(dtype)
        if dtype not in _DST:
            raise TypeError(f"a frame cannot be materialised as {dtype}")
        if self.dtype not in _SRC:
            raise TypeError(f"a {self.dtype} frame cannot be gathered again")
        G, C = self.shape
        buf = _lib.DeviceBuffer(max(G * C * dtype.itemsize, 16), self.device_id)
        bad = ctypes.c_int64()
        try:
            _lib.check(_lib.lib().cyto_select(*self._view_args(), buf.ptr, C, _DST[dtype], ctypes.byref(bad), self.device_id, None))
            if bad.value and not allow_inexact and dtype != self.dtype:     # (a same-type gather copies the bits: its "inexact" are NaNs)
                raise ValueError(f"{bad.value} values of the frame do not convert to {dtype} exactly")
        except BaseException:
            buf.free()
            raise
        self.stats["materialized"] += 1
        return DeviceFrame(buf, (G, C), C, dtype, self._index, self._columns, None, None, self.device_id, self.stats)

    def materialize(self, dtype=None):
        """The view as a frame of its own: a fresh contiguous buffer (ld == columns) of `dtype` (None: this frame's), gathered and
        converted on the device (cyto_select).  ValueError when a value does not survive the conversion to ANOTHER dtype."""
        return self._select(dtype)

    def value_range(self):
        """cyto_value_range of the view: {"lo", "hi" (floats; exact ints for an integer frame), "non_integral", "non_finite",
        "not_f32_exact"}."""
        lo, hi = ctypes.c_double(), ctypes.c_double()
        ilo, ihi, nint, nfin, n32 = (ctypes.c_int64() for _ in range(5))
        _lib.check(_lib.lib().cyto_value_range(*self._view_args(), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(ilo), ctypes.byref(ihi),
                                               ctypes.byref(nint), ctypes.byref(nfin), ctypes.byref(n32), self.device_id, None))
        ints = self.dtype.kind in "iu"
        return {"lo": ilo.value if ints else lo.value, "hi": ihi.value if ints else hi.value, "non_integral": nint.value,
                "non_finite": nfin.value, "not_f32_exact": n32.value}

    def narrowest(self):
        """The dtype cytospace._counts_matrix would choose for this view's values (one pass on the device; none for a float32 /
        uint16 / uint8 frame, which stays what it is)."""
        if self.dtype in (np.dtype(np.float32), np.dtype(np.uint8), np.dtype(np.uint16)):
            return self.dtype
        r = self.value_range()
        return narrowest_dtype(self.dtype, r["lo"], r["hi"], r["non_integral"], r["not_f32_exact"])

    def to_numpy(self):
        """The view's values on the host (a download; counted in `fetches`)."""
        G, C = self.shape
        self.stats["fetches"] += 1
        if G == 0 or C == 0:
            return np.empty((G, C), self.dtype)
        if self._rows is None and self._cols is None and self._ld == self._shape[1]:
            out = np.empty((G, C), self.dtype)
            _lib.check(_lib.lib().cyto_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, self.device_id))
            return out
        m = self._select(None, allow_inexact=True)          # (a same-type gather copies the bits; "inexact" are its NaNs)
        self.stats["materialized"] -= 1                       # (part of the fetch, not a stage's matrix)
        try:
            return m._owner.to_numpy((G, C), self.dtype)
        finally:
            m.close()

    def to_frame(self):
        """The DataFrame the host path would hold at this point: same index, columns, dtypes and values.  Each call downloads
        (`fetches` += 1)."""
        import pandas as pd
        return pd.DataFrame(self.to_numpy(), index=self._index, columns=self._columns, copy=False)

    @classmethod
    def from_frame(cls, df, device_id=0):
        """Upload a DataFrame of one dtype (int64, float64, uint16 or float32) with unique column labels; TypeError for any other
        (the caller keeps the DataFrame)."""
        if not df.columns.is_unique:
            raise TypeError("duplicate column labels")
        kinds = df.dtypes.unique()
        if len(kinds) != 1 or np.dtype(kinds[0]) not in _SRC:
            raise TypeError(f"dtypes {[str(k) for k in kinds]}")
        x = np.ascontiguousarray(df.to_numpy())
        buf = _lib.DeviceBuffer(max(x.nbytes, 16), device_id)
        if x.nbytes:
            _lib.check(_lib.lib().cyto_memcpy_h2d(buf.ptr, x.ctypes.data, x.nbytes, device_id))
        return cls(buf, x.shape, x.shape[1], x.dtype, df.index, df.columns, device_id=device_id, source="upload")

    def close(self):
        """Free the buffer (every frame taken from this one loses it too)."""
        self._owner.free()

    def __repr__(self):
        return f"DeviceFrame({self.shape[0]} x {self.shape[1]} {self.dtype}, source={self.source!r}, device={self.device_id})"


def from_table(handle, G, head, is_float, labels, sep, device_id, info):
    """read_file_device's resident result: the frame over a parsed table's own values (handle: cyto_table, owned by the frame
    from here on), or None when a frame cannot stand for it (mixed column kinds, duplicate column labels, row labels outside the
    grammar: info["reason"]) -- the caller then fetches the values and frees the handle as before."""
    from .common import _table_frame
    f = np.asarray(is_float).astype(bool)
    if f.any() and not f.all():
        info["resident_reason"] = "mixed column kinds"
        return None
    if not head.columns.is_unique:
        info["resident_reason"] = "duplicate column labels"
        return None
    # the labels go through the host path's own code: the frame of a table without values
    empty = _table_frame(head.iloc[:, :0], np.empty((int(G), 0), np.int64), f[:0], labels, sep, info)
    if empty is None:
        return None
    owner = _Table(handle, device_id)
    dtype = np.float64 if f.all() else np.int64
    return DeviceFrame(owner, (len(empty.index), len(head.columns)), owner.ld, dtype, empty.index, head.columns, device_id=device_id,
                       source="table")
