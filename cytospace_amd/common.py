"""Device-backed counterparts of the reference's numeric helpers (cytospace/common/common.py).

Same names, argument meaning and error behaviour; the arithmetic runs in HIP kernels
(cytospace_amd/csrc/cost.hip) through the C ABI.  No numpy fallback exists.
"""
import ctypes

import numpy as np

from . import _lib

_BK, _BM = 32, 128


def _as_matrix(a):
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("expected a 2-D genes x columns matrix")
    if a.dtype == np.float32:
        return np.ascontiguousarray(a), 0
    if a.dtype == np.uint16:                       # (raw counts: CYTO_DTYPE_U16 / _U8, widened on the device)
        return np.ascontiguousarray(a), 2
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a), 3
    return np.ascontiguousarray(a, dtype=np.float64), 1


def normalize_data(data, device_id=0):
    """cytospace/common/common.py:142-147 on the GPU: nan_to_num, per-column CPM, log2(x+1).
    Returns a float64 array like the reference."""
    x, is64 = _as_matrix(data)
    G, C = x.shape
    out = np.empty((G, C), np.float64)
    _lib.check(_lib.lib().cyto_normalize_data(G, C, x.ctypes.data, C, is64, out.ctypes.data, C, device_id))
    return out


def normalized_column_sums(data, device_id=0, return_kernel_ms=False):
    """`normalize_data(data).sum(axis=0, dtype=float)` -- the same float64[C], bit for bit -- computed on the GPU without the
    normalised matrix (C ABI: cyto_normalized_colsums): the counts go up in the narrowest dtype that holds them
    (cytospace._counts_matrix) and C doubles come back.  data: a 2-D genes x columns array, or a resident.DeviceFrame, which is read
    where it lies (gathered on the device first when it is a view or of another dtype than its narrowest; nothing is fetched).
    return_kernel_ms: also return the HIP-event time of the summing kernel.

    The kernel adds a column's genes in ascending order, which is numpy's order whenever there are two columns or more.  A table of
    ONE column is a contiguous vector to numpy, which adds such a vector pairwise, in blocks that depend on its buffer size: there
    numpy itself adds the G numbers of normalize_data (the values are fetched if they are a DeviceFrame's; kernel time 0)."""
    from . import cytospace, resident
    mat = None
    if not resident.is_frame(data):
        data = np.asarray(data)
    if data.shape[1:] == (1,) and data.shape[0] > 0:
        x = data.to_numpy() if resident.is_frame(data) else data
        out = normalize_data(x.astype(float), device_id).sum(axis=0, dtype=float)
        return (out, 0.0) if return_kernel_ms else out
    if resident.is_frame(data):
        G, C = data.shape
        if G > 0 and C > 0:
            m, mat = cytospace._resident_matrix(data)
    else:
        x = np.asarray(data)
        if x.ndim != 2:
            raise ValueError("expected a 2-D genes x columns matrix")
        x, code = cytospace._boundary_matrix(cytospace._counts_matrix(x))
        G, C = x.shape
        m = cytospace._matrix_struct(x, code)
    if G <= 0 or C <= 0:
        raise ValueError("expected a genes x columns matrix with at least one gene and one column")
    out = np.empty(C, np.float64)
    ms = ctypes.c_double()
    try:
        _lib.check(_lib.lib().cyto_normalized_colsums_timed(G, C, ctypes.byref(m), out.ctypes.data, device_id, None,
                                                            ctypes.byref(ms) if return_kernel_ms else None))
    finally:
        if mat is not None:
            mat.close()
    return (out, ms.value) if return_kernel_ms else out


METRICS ={"Pearson_correlation": 0, "Spearman_correlation": 1, "Euclidean": 2}   # CYTO_METRIC_*


def is_sparse(x):
    try:
        import scipy.sparse as sp
    except ImportError:
        return False
    return sp.issparse(x)


def sparse_to_device(x, device_id=0):
    """A scipy.sparse genes x columns count matrix -> dense float32 G x ld matrix in HBM (C ABI: cyto_csc_to_dense_f32): only the
    non-zeros cross PCIe and the expansion runs on the device.  The reference densifies on the host
    (`pd.DataFrame.sparse.from_spmatrix(...).sparse.to_dense()`, cytospace/common/common.py:57).
    Returns (DeviceBuffer, G, C, ld).  Values must be exact in float32 (counts are)."""
    csc = x.tocsc()
    csc.sum_duplicates()
    G, C = csc.shape
    vals = np.ascontiguousarray(csc.data, dtype=np.float32)
    if not np.array_equal(vals.astype(csc.data.dtype, copy=False), csc.data):
        raise ValueError("sparse values are not exactly representable in float32; pass a dense float64 matrix instead")
    colptr = np.ascontiguousarray(csc.indptr, dtype=np.int64)
    rowidx = np.ascontiguousarray(csc.indices, dtype=np.int32)
    ld = -(-C // 4) * 4
    buf = _lib.DeviceBuffer(max(G, 1) * ld * 4, device_id)
    _lib.check(_lib.lib().cyto_csc_to_dense_f32(G, C, len(vals), colptr.ctypes.data, rowidx.ctypes.data if len(vals) else None,
                                                vals.ctypes.data if len(vals) else None, buf.ptr, ld, device_id, None))
    return buf, G, C, ld


def read_file(file_path, keep_sparse=True):
    """cytospace/common/common.py:16-82.  A MatrixMarket file (.mtx / .mtx.gz, genes x cells, with genes|features and
    cells|barcodes lists beside it) or a delimited text table (.csv: ','; otherwise tab) with gene ids in the first column.
    Returns a pandas DataFrame like the reference -- except that, with keep_sparse, a MatrixMarket input stays sparse
    (a DataFrame of pandas sparse columns, `df.sparse.to_coo()` recovers the matrix): ExpressionContext uploads it as non-zeros."""
    import os
    import pandas as pd
    if file_path.endswith(".mtx") or file_path.endswith(".mtx.gz"):
        import scipy.io
        if not os.path.isfile(file_path):
            raise IOError("Cannot locate file: {}".format(file_path))
        genes, cells, gpath, cpath = _mtx_labels(file_path)
        m = scipy.io.mmread(file_path)
        if m.shape != (len(genes), len(cells)):
            raise IOError("The dimensions of the provided sparse matrix does not match the corresponding gene and cell lists. "
                          f"Please check the following files: {gpath}, {cpath}.")
        df = pd.DataFrame.sparse.from_spmatrix(m, index=genes, columns=cells)
        return df if keep_sparse else df.sparse.to_dense()
    sep = "," if file_path.lower().endswith(".csv") else "\t"
    return pd.read_csv(file_path, sep=sep, header=0, index_col=0)


def _mtx_labels(file_path):
    """The gene and cell lists beside a MatrixMarket file (genes|features and cells|barcodes, .tsv / .csv, plain or .gz), as
    cytospace/common/common.py:27-52 reads them: (genes, cells, genes' path, cells' path).  IOError if one is missing."""
    import os
    import pandas as pd
    base = os.path.dirname(file_path) + os.path.sep

    def find(names):
        for name in names:
            for ext in (".tsv", ".csv", ".tsv.gz", ".csv.gz"):
                if os.path.isfile(f"{base}{name}{ext}"):
                    return f"{base}{name}{ext}", ext
        raise IOError(f"Required files not found for base path: {base}")
    gpath, gext = find(["genes", "features"])
    cpath, cext = find(["cells", "barcodes"])
    genes = pd.read_csv(gpath, sep="\t" if ".tsv" in gext else ",", header=None).iloc[:, 0].to_numpy()
    cells = pd.read_csv(cpath, sep="\t" if ".tsv" in cext else ",", header=None).iloc[:, 0].to_numpy()
    return genes, cells, gpath, cpath


# why cyto_table_read refused a file (CYTO_TABLE_ERR_*): read_file_device's info["reason"]["kind"]
_TABLE_REFUSALS = {1: "io", 2: "control byte", 3: "quote", 4: "carriage return", 5: "blank line", 6: "field count", 7: "token",
                   8: "out of range", 9: "integer cast in a float column"}
_COMPRESSED = (".gz", ".bz2", ".zip", ".xz", ".zst", ".tar")
# a row label that pandas would not keep as text (a number, inf / nan, a boolean): in an object index it may come out as text here
# but as a number in pandas' own read, which infers types per block of rows
_NOT_TEXT = r"\s*[+-]?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?|inf|infinity|nan)\s*|true|false"
# an integer label whose value may differ between a block of rows read as int64 and one read as float64 (17+ digits, "-0")
_CAST_LABEL = r"\s*[+-]?\d{17,}\s*|\s*-0+\s*"


def _table_head(header, first, sep, C):
    """pandas' parse of the header line with the first data line (it decides between the two header shapes): a frame of one row
    whose columns and index name are the table's; None if pandas refuses it or does not see C data columns."""
    import io
    import pandas as pd
    try:
        head = pd.read_csv(io.BytesIO(header + first), sep=sep, header=0, index_col=0)
    except Exception:
        return None
    if head.shape[1] != C or isinstance(head.index, pd.MultiIndex):
        return None
    return head


def _table_on_device(file_path, device_id, info, resident=False):
    """read_file_device's device path: the DataFrame, or None (info["reason"] says why) for a file outside its grammar.  resident:
    a resident.DeviceFrame over the parsed values where a frame can stand for the table (only the labels are fetched and the
    handle stays with the frame), else the DataFrame as before (info["resident_reason"] says why)."""
    import time

    def refuse(kind, line=0, byte=0):
        info["reason"] = {"kind": kind, "line": int(line), "byte": int(byte)}
        return None
    if not isinstance(file_path, str):
        return refuse("not a path")
    low = file_path.lower()
    if file_path.endswith(".mtx") or file_path.endswith(".mtx.gz"):
        return refuse("matrix market")
    if low.endswith(_COMPRESSED):
        return refuse("compressed")
    sep = "," if low.endswith(".csv") else "\t"
    try:
        with open(file_path, "rb") as f:
            header, first = f.readline(), f.readline()
    except OSError:
        return refuse("io")
    # the header goes to pandas as it is; it must be one line to pandas too (no '\r' but before its '\n', no open quote)
    name_line = header[:-2] if header.endswith(b"\r\n") else header[:-1]
    if not header.endswith(b"\n") or not name_line.strip() or b"\r" in name_line or name_line.count(b'"') % 2 or \
            any(b < 0x20 and b != ord(sep) for b in name_line):
        return refuse("header", 1)
    C = first.count(sep.encode())
    if C == 0:
        return refuse("no data columns", 2)
    t = time.perf_counter()
    head = _table_head(header, first, sep, C)
    if head is None:
        return refuse("header", 1)
    info["header_s"] = time.perf_counter() - t
    L = _lib.lib()
    h = ctypes.c_void_p()
    shape, why = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    ms, ms_dl = (ctypes.c_double * 3)(), ctypes.c_double()
    t = time.perf_counter()
    st = L.cyto_table_read(file_path.encode(), sep.encode(), len(header), C, device_id, ctypes.byref(h), shape, why, ms)
    call = time.perf_counter() - t
    info.update(file_read_s=ms[0] / 1e3, upload_s=ms[1] / 1e3, kernels_s=ms[2] / 1e3)
    info["device_setup_s"] = max(0.0, call - (ms[0] + ms[1] + ms[2]) / 1e3)     # allocations, pinned buffers, their release
    if st == 7:                                                              # CYTO_ERR_UNSUPPORTED
        return refuse(_TABLE_REFUSALS.get(why[0], str(why[0])), why[1], why[2])
    _lib.check(st)
    if resident:
        from . import resident as _resident
        frame = None
        try:
            G, C, nlab = shape
            is_float = np.empty(C, np.int8)
            labels = np.empty(nlab, np.uint8)
            _lib.check(L.cyto_table_fetch_labels(h, is_float.ctypes.data, labels.ctypes.data, ctypes.byref(ms_dl)))
            info["download_s"] = ms_dl.value / 1e3
            frame = _resident.from_table(h, G, head, is_float, labels, sep, device_id, info)
        except BaseException:
            L.cyto_table_free(h)
            raise
        if frame is not None:
            info["resident"] = True
            return frame
        if "reason" in info:                             # (row labels outside the grammar: pandas reads the file)
            L.cyto_table_free(h)
            return None
    try:
        G, C, nlab = shape
        values = np.empty((G, C), np.int64)
        is_float = np.empty(C, np.int8)
        labels = np.empty(nlab, np.uint8)
        _lib.check(L.cyto_table_fetch(h, values.ctypes.data, is_float.ctypes.data, labels.ctypes.data, ctypes.byref(ms_dl)))
    finally:
        t = time.perf_counter()
        L.cyto_table_free(h)
        info["free_s"] = time.perf_counter() - t
    info["download_s"] = ms_dl.value / 1e3
    return _table_frame(head, values, is_float, labels, sep, info)


def _table_frame(head, values, is_float, labels, sep, info):
    """The DataFrame of _table_on_device from what cyto_table_fetch gave (values: G x C int64 words, is_float: C flags, labels:
    the packed row labels) and pandas' parse of the header; or None (info["reason"]) when the row labels are outside the grammar."""
    import io
    import time
    import pandas as pd

    def refuse(kind, line=0, byte=0):
        info["reason"] = {"kind": kind, "line": int(line), "byte": int(byte)}
        return None
    t = time.perf_counter()
    # the row labels, handed back to pandas as a table of their own: its inference (integers, NA, ...), duplicates kept
    index = pd.read_csv(io.BytesIO(labels.tobytes()), sep=sep, header=None, index_col=0).index
    if index.dtype == object and pd.Series(index.astype(str)).str.fullmatch(_NOT_TEXT, case=False).any():
        return refuse("row labels")
    if index.dtype.kind in "fu" and pd.Series(labels.tobytes().decode("utf-8", "replace").split(sep + "\n")[:-1]).str.fullmatch(
            _CAST_LABEL).any():
        return refuse("row labels")
    index = index.rename(head.index.name)
    f = is_float.astype(bool)
    if not f.any():
        df = pd.DataFrame(values, index=index, columns=head.columns, copy=False)
    elif f.all():
        df = pd.DataFrame(values.view(np.float64), index=index, columns=head.columns, copy=False)
    else:
        df = pd.concat([pd.DataFrame(values[:, ~f]), pd.DataFrame(values[:, f].view(np.float64))], axis=1, ignore_index=True)
        df = df.iloc[:, np.argsort(np.concatenate([np.flatnonzero(~f), np.flatnonzero(f)]), kind="stable")]
        df.index, df.columns = index, head.columns
    info["dataframe_s"] = time.perf_counter() - t
    return df


def read_file_device(file_path, device_id=0, return_info=False, resident=False):
    """read_file(file_path, keep_sparse=False) for a dense delimited text table (.csv: ','; otherwise tab), parsed on the GPU
    (C ABI: cyto_table_read / cyto_table_fetch; csrc/table.hip).  The result is equal to read_file's: index, columns (pandas'
    header parse, duplicates mangled), every column's dtype (int64 or float64) and every value bit for bit (pandas' own decimal
    converter).  A file outside the grammar of DESIGN.md 4.1c -- quotes, NA or empty values, ragged or blank lines, numbers with 19+
    digits before the point, values beyond float64, MatrixMarket, compressed files, no data columns -- is read by read_file itself: its result, or
    its exception.

    return_info: also return a dict -- "path" ("device" or "pandas"), for a fallback "reason" {"kind", "line", "byte"}, and the
    phase times in seconds: header_s (pandas' parse of the header), file_read_s, upload_s (what the upload added to the reads),
    kernels_s, device_setup_s (the rest of the device call: allocations, pinned buffers, their release), download_s, free_s,
    dataframe_s (the row labels' parse and the DataFrame), total_s.

    resident=True: a table the device path takes whose columns are all int64 or all float64, with unique column labels, comes
    back as a resident.DeviceFrame -- the values stay in HBM, only the labels are fetched, `.to_frame()` is the DataFrame above.
    Every other input gives the DataFrame as before.  info["resident"] says which (for a DataFrame, info["resident_reason"] why)."""
    import time
    t = time.perf_counter()
    info = {"path": "device", "resident": False}
    df = _table_on_device(file_path, device_id, info, resident)
    if df is None:
        info["path"] = "pandas"
        df = read_file(file_path, keep_sparse=False)
    info["total_s"] = time.perf_counter() - t
    return (df, info) if return_info else df


def parse_table_tokens(tokens):
    """The device reader's token converter, run on the host (C ABI: cyto_table_parse_tokens, a test hook).  tokens: a list of
    str.  Returns (kind, value, ints): kind 0 integer token, 1 decimal token, 2 outside the token grammar, 3 out of range; value
    the float64 as the converter gives it (kinds 0 and 1); ints the int64 value (kind 0)."""
    raw = [t.encode() for t in tokens]
    text = b"".join(raw)
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    n = len(raw)
    kind, value, ints = np.empty(n, np.int8), np.empty(n, np.float64), np.empty(n, np.int64)
    buf = ctypes.create_string_buffer(text, len(text) + 1)
    _lib.check(_lib.lib().cyto_table_parse_tokens(buf, n, off.ctypes.data, value.ctypes.data, ints.ctypes.data, kind.ctypes.data))
    return kind, value, ints


# why cyto_mtx_read refused a body (CYTO_MTXR_ERR_*): read_mtx_device's info["reason"]["kind"]
_MTX_REFUSALS = {1: "io", 2: "byte", 3: "carriage return", 4: "entry count", 5: "blank line", 6: "fields", 7: "index", 8: "token",
                 9: "inexact", 10: "negative zero", 11: "duplicate entry", 12: "memory"}
_MTX_HEAD_BYTES = 1 << 20
# scipy's reader wants the banner's first word as it is spelt; the other words in any case
_MTX_BANNER = rb"%%MatrixMarket(?i:[ \t]+matrix[ \t]+coordinate[ \t]+(integer|real)[ \t]+general)[ \t]*\r?\n"
_MTX_SIZE = rb"[ \t]*(\d{1,18})[ \t]+(\d{1,18})[ \t]+(\d{1,18})[ \t]*(\r?\n)?"


def parse_mtx_header(head, file_size):
    """The header of a MatrixMarket file inside the device grammar, from the file's first bytes `head` (at most
    the first MiB is looked at): the banner `%%MatrixMarket matrix coordinate integer|real general`, lines starting with '%', then
    the size line of three [0-9]{1,18} tokens.  Returns {"field": 0 integer / 1 real, "G", "C", "nnz", "data_offset", "lines"} --
    or the 1-based line at which the header leaves the grammar (another format or symmetry, a blank line, G or C of 0, a size line
    that is not three such tokens, no size line within the first MiB)."""
    import re
    head = bytes(head[:_MTX_HEAD_BYTES])
    end = head.find(b"\n") + 1
    m = re.fullmatch(_MTX_BANNER, head[:end]) if end else None
    if m is None:
        return 1
    field = 0 if m.group(1).lower() == b"integer" else 1
    line = 1
    while True:
        line += 1
        start, end = end, head.find(b"\n", end) + 1
        if not end:                                       # no line end: the size line of a file that stops there, or nothing
            end = len(head)
            if end != file_size or end == start:
                return line
        if head[start:start + 1] == b"%":
            if head[end - 1:end] != b"\n":
                return line
            continue
        m = re.fullmatch(_MTX_SIZE, head[start:end])
        if m is None:
            return line
        G, C, nnz = (int(m.group(k)) for k in (1, 2, 3))
        if G == 0 or C == 0:
            return line
        return {"field": field, "G": G, "C": C, "nnz": nnz, "data_offset": end, "lines": line}


def _mtx_frame(genes, cells, words, field):
    """read_mtx_device's DataFrame from the label lists and the G x C result words (int64 values, or float64 bits for field 1)."""
    import pandas as pd
    return pd.DataFrame(words if field == 0 else words.view(np.float64), index=genes, columns=cells, copy=False)


def _mtx_on_device(file_path, device_id, info):
    """read_mtx_device's device path: the DataFrame, or None (info["reason"] says why) for a file outside its grammar."""
    import os
    import time
    import pandas as pd

    def refuse(kind, line=0, byte=0):
        info["reason"] = {"kind": kind, "line": int(line), "byte": int(byte)}
        return None
    if not isinstance(file_path, str):
        return refuse("not a path")
    if file_path.endswith(".mtx.gz"):
        return refuse("compressed")
    if not file_path.endswith(".mtx"):
        return refuse("not matrix market")
    if not os.path.isfile(file_path):
        return refuse("io")
    t = time.perf_counter()
    try:
        genes, cells, _, _ = _mtx_labels(file_path)
        # (DataFrame.sparse.to_dense goes through a dict keyed by column label: with a repeated or missing label it is not the matrix)
        if pd.Index(cells).has_duplicates or pd.isna(cells).any():
            return refuse("labels")
    except Exception:
        return refuse("labels")
    info["labels_s"] = time.perf_counter() - t
    t = time.perf_counter()
    try:
        with open(file_path, "rb") as f:
            head = f.read(_MTX_HEAD_BYTES)
            size = os.fstat(f.fileno()).st_size
    except OSError:
        return refuse("io")
    h = parse_mtx_header(head, size)
    info["header_s"] = time.perf_counter() - t
    if not isinstance(h, dict):
        return refuse("header", h)
    if (h["G"], h["C"]) != (len(genes), len(cells)):
        return refuse("shape", h["lines"])
    try:
        words = np.empty((h["G"], h["C"]), np.int64)
    except MemoryError:
        return refuse("memory")
    r = _lib.MtxReadInfo()
    st = _lib.lib().cyto_mtx_read(file_path.encode(), h["data_offset"], h["G"], h["C"], h["nnz"], h["field"], words.ctypes.data,
                                  h["C"], device_id, ctypes.byref(r))
    info.update(file_read_s=r.ms_read / 1e3, upload_s=r.ms_upload / 1e3, kernels_s=r.ms_kernels / 1e3, download_s=r.ms_download / 1e3)
    if st == _lib.CYTO_ERR_UNSUPPORTED:
        return refuse(_MTX_REFUSALS.get(r.reason_kind, str(r.reason_kind)), r.reason_line, r.reason_byte)
    if st == 3:                                                              # CYTO_ERR_NOMEM
        return refuse("memory")
    _lib.check(st)
    info.update(field="integer" if h["field"] == 0 else "real", entries=int(r.entries), duplicates=int(r.duplicates))
    t = time.perf_counter()
    df = _mtx_frame(genes, cells, words, h["field"])
    info["dataframe_s"] = time.perf_counter() - t
    return df


def read_mtx_device(file_path, device_id=0, return_info=False):
    """read_file(file_path, keep_sparse=False) for a MatrixMarket `.mtx` file with its genes|features and cells|barcodes lists
    beside it, the body parsed and made dense on the GPU (C ABI: cyto_mtx_read; csrc/mtx_read.hip).  The result is equal to
    read_file's: the index from the gene list, the columns from the cell list (both read by the pd.read_csv calls of read_file),
    every column int64 for an `integer` file and float64 for a `real` one, every value bit for bit, duplicate entries of an
    integer file summed.  A file outside the grammar of DESIGN.md 4.1e -- `.mtx.gz`, another banner than `coordinate integer|real
    general`, a body with empty lines, comments, a `+`, values scipy's converter would have to round twice, negative zeros,
    duplicate entries in a real file, repeated cell labels -- and every file read_file raises for (missing, without its lists, a
    size line that disagrees with them, a malformed body) is read by read_file itself: its result, or its exception.

    return_info: also return a dict -- "path" ("device" or "scipy"), for a fallback "reason" {"kind", "line", "byte"}, for the
    device path "field" ("integer" / "real"), "entries" and "duplicates" (entries that met a non-zero sum in their cell), and the
    phase times in seconds: labels_s (the two lists), header_s, file_read_s, upload_s (what the upload added to the reads),
    kernels_s (zero fill included), download_s, dataframe_s, total_s."""
    import time
    t = time.perf_counter()
    info = {"path": "device"}
    df = _mtx_on_device(file_path, device_id, info)
    if df is None:
        info["path"] = "scipy"
        df = read_file(file_path, keep_sparse=False)
    info["total_s"] = time.perf_counter() - t
    return (df, info) if return_info else df


def parse_mtx_entries(lines, field, G, C):
    """The device reader's entry-line parser, run on the host (C ABI: cyto_mtx_parse_entries, a test hook).  lines: a list of
    bytes, each an entry line without its line end; field 0 integer / 1 real.  Returns (kind, where, row, col, value): kind 0 or
    the CYTO_MTXR_ERR_* code, where the offset in the line that the refusal names, row and col 1-based, value the int64 value or
    the float64 bits."""
    text = b"".join(lines)
    n = len(lines)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in lines], out=off[1:])
    kind = np.empty(n, np.int8)
    where, row, col, value = (np.empty(n, np.int64) for _ in range(4))
    buf = ctypes.create_string_buffer(text, len(text) + 1)
    _lib.check(_lib.lib().cyto_mtx_parse_entries(buf, n, off.ctypes.data, field, G, C, kind.ctypes.data, where.ctypes.data,
                                                 row.ctypes.data, col.ctypes.data, value.ctypes.data))
    return kind, where, row, col, value


def downsample(data_df, target_count):
    """cytospace/common/common.py:149-173.  Every cell (column) with more than target_count transcripts is reduced to
    target_count draws WITH replacement from its transcripts (np.random.choice over the expanded gene list, legacy
    RandomState: same draws as the reference for the same np.random.seed); other cells are kept.  Host code."""
    import pandas as pd
    index = data_df.index
    values = data_df.to_numpy()
    out = np.array(values, copy=True)
    for c in range(values.shape[1]):
        col = values[:, c]
        if col.sum() <= target_count:
            continue
        picked = np.random.choice(np.repeat(np.arange(len(index)), col), target_count)
        out[:, c] = np.bincount(picked, minlength=len(index))
    return pd.DataFrame(out, index=index, columns=data_df.columns)


# upload codes of cyto_downsample (CYTO_DTYPE_*); other integer dtypes are widened on the host first
_DS_IN = {np.dtype(np.uint8): 3, np.dtype(np.uint16): 2, np.dtype(np.int32): 4, np.dtype(np.int64): 5}
_DS_WIDEN = {np.dtype(np.bool_): np.uint8, np.dtype(np.int8): np.int32, np.dtype(np.int16): np.int32, np.dtype(np.uint32): np.int64}


def downsample_device(data_df, target_count, device_id=0, dtype=np.int64, return_words=False):
    """`downsample` on the GPU (C ABI: cyto_downsample): the same DataFrame -- index, columns, values -- and the same
    global numpy RandomState afterwards (np.random.set_state keeps has_gauss and the cached value), for the same state
    before.  The draws follow numpy's legacy MT19937 stream and masked rejection sampling word for word.

    dtype: np.int64 (default) or np.uint16 (target_count < 65536 and no negative count: every value is then at most
    target_count).  return_words: also return the number of raw MT19937 words consumed.  Raises TypeError for a non-integer matrix (np.repeat refuses it) and ValueError, before any draw,
    for a negative count in a cell that is downsampled or a cell total above 2^32."""
    import pandas as pd
    from . import resident as _resident
    frame = data_df if _resident.is_frame(data_df) else None
    x = np.empty((0, 0), frame.dtype) if frame is not None else data_df.to_numpy()
    if x.dtype.kind not in "biu" or x.dtype == np.uint64:
        raise TypeError(f"Cannot downsample counts of dtype {x.dtype}: an integer count matrix is required")
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.int64), np.dtype(np.uint16)):
        raise ValueError("dtype must be np.int64 or np.uint16")
    target = int(target_count)
    if target < 0:
        raise ValueError("target_count must be non-negative")
    if dtype == np.uint16 and target > 65535:
        raise ValueError("dtype=np.uint16 needs target_count < 65536")
    if target > 2**31 - 1:
        raise ValueError("target_count must be below 2^31")
    G, C = data_df.shape
    if frame is not None and (G == 0 or C == 0):
        x = frame.to_numpy()
    if G == 0 or C == 0:
        df = pd.DataFrame(x.astype(dtype), index=data_df.index, columns=data_df.columns)
        if frame is not None:
            df = _resident.DeviceFrame.from_frame(df.astype(dtype), device_id)
        return (df, 0) if return_words else df
    if frame is not None:
        return _downsample_frame(frame, target, device_id, dtype, return_words)
    if x.dtype in _DS_WIDEN:
        x = x.astype(_DS_WIDEN[x.dtype])
    x = np.ascontiguousarray(x)
    state = np.random.get_state()
    if state[0] != "MT19937":
        raise ValueError("numpy's global generator is not MT19937")
    key = np.array(state[1], dtype=np.uint32)
    pos = ctypes.c_int32(int(state[2]))
    words = ctypes.c_int64()
    out = np.empty((G, C), dtype)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    st = _lib.lib().cyto_downsample(G, C, x.ctypes.data, C, _DS_IN[x.dtype], out.ctypes.data, C, 5 if dtype == np.int64 else 2, target,
                                    key.ctypes.data_as(u32p), ctypes.byref(pos), ctypes.byref(words), device_id)
    if st == 1:
        raise ValueError("cannot downsample: a cell with more than target_count transcripts holds a negative count or more than "
                         "2^32 transcripts" + (" (or, with dtype=np.uint16, some count is negative)" if dtype == np.uint16 else ""))
    _lib.check(st)
    np.random.set_state(("MT19937", key, pos.value, state[3], state[4]))
    df = pd.DataFrame(out, index=data_df.index, columns=data_df.columns)
    return (df, words.value) if return_words else df


def _downsample_frame(frame, target, device_id, dtype, return_words):
    """downsample_device for a resident.DeviceFrame: the view is materialised to int64 on the device, cyto_downsample_dev writes
    a second buffer, and the result is the frame over it; only the cells' totals and the generator's state cross PCIe."""
    from . import resident as _resident
    G, C = frame.shape
    state = np.random.get_state()
    if state[0] != "MT19937":
        raise ValueError("numpy's global generator is not MT19937")
    key = np.array(state[1], dtype=np.uint32)
    pos = ctypes.c_int32(int(state[2]))
    words = ctypes.c_int64()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    x = frame.materialize(np.int64)
    out = _lib.DeviceBuffer(G * C * dtype.itemsize, device_id)
    try:
        st = _lib.lib().cyto_downsample_dev(G, C, x.ptr, x.ld, _lib.CYTO_DTYPE_I64, out.ptr, C, 5 if dtype == np.int64 else 2, target,
                                            key.ctypes.data_as(u32p), ctypes.byref(pos), ctypes.byref(words), device_id)
        if st == 1:
            raise ValueError("cannot downsample: a cell with more than target_count transcripts holds a negative count or more than "
                             "2^32 transcripts" + (" (or, with dtype=np.uint16, some count is negative)" if dtype == np.uint16 else ""))
        _lib.check(st)
    except BaseException:
        out.free()
        raise
    finally:
        x.close()
    np.random.set_state(("MT19937", key, pos.value, state[3], state[4]))
    res = _resident.DeviceFrame(out, (G, C), C, dtype, frame.index, frame.columns, device_id=device_id, stats=frame.stats)
    return (res, words.value) if return_words else res


# upload codes of cyto_placeholders; other dtypes are widened on the host first (to what numpy's float64 assignment sees anyway)
_PH_IN = {np.dtype(np.int64): 5, np.dtype(np.uint16): 2, np.dtype(np.float64): 1}
_PH_WIDEN = {np.dtype(t): np.int64 for t in (np.int8, np.int16, np.int32, np.uint8, np.uint32)}
_PH_WIDEN[np.dtype(np.float32)] = np.float64


def place_holders_device(own, short, device_id=0, return_words=False, rbuf_bytes=0):
    """The synthetic cells of sample_single_cells' "place_holders" branch on the GPU (C ABI: cyto_placeholders): for the G x n
    matrix `own` of a cell type's cells, the G x short float64 array of the host loop

        fake[:, k] = [np.random.choice(own[g, :]) for g in range(G)]          k = 0 .. short-1

    and the same global numpy RandomState afterwards (np.random.set_state keeps has_gauss and the cached value).  That loop
    consumes the stream of np.random.randint(0, n, size=(short, G)) -- masked rejection sampling on 32-bit MT19937 words, no
    word at all when n == 1 -- which the device reproduces word for word.

    own: int64, uint16 or float64 as they are (rows may be strided); narrower integers are widened to int64 and float32 to
    float64 first; any other dtype raises TypeError.  return_words: also return the number of raw words consumed.
    rbuf_bytes: a cap on one block's draws (0: the library's default); results do not depend on it."""
    out, state, words = place_holders_from_state(own, short, np.random.get_state(), device_id, rbuf_bytes)
    np.random.set_state(state)
    return (out, words) if return_words else out


def place_holders_from_state(own, short, state, device_id=0, rbuf_bytes=0):
    """place_holders_device on an explicit legacy state tuple (np.random.get_state()) instead of numpy's global one: returns
    (the G x short array, the state after the draws, words consumed).  Touches nothing global, so host threads may call it
    side by side, each with a state of its own."""
    own = np.asarray(own)
    if own.ndim != 2:
        raise ValueError("own must be a genes x cells matrix")
    if own.dtype in _PH_WIDEN:
        own = own.astype(_PH_WIDEN[own.dtype])
    if own.dtype not in _PH_IN:
        raise TypeError(f"Cannot draw place-holder cells from values of dtype {own.dtype}")
    short = int(short)
    if short < 0:
        raise ValueError("short must be non-negative")
    G, n = own.shape
    if n == 0 and G > 0 and short > 0:
        raise ValueError("a cell type without cells has nothing to draw from")        # (np.random.choice([]) raises as well)
    out = np.empty((G, short), np.float64)
    if state[0] != "MT19937":
        raise ValueError("numpy's global generator is not MT19937")
    if G == 0 or short == 0:
        return out, state, 0
    item = own.dtype.itemsize
    if own.strides[1] != item or own.strides[0] % item or own.strides[0] < n * item:
        own = np.ascontiguousarray(own)
    key = np.array(state[1], dtype=np.uint32)
    pos = ctypes.c_int32(int(state[2]))
    words = ctypes.c_int64()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    _lib.check(_lib.lib().cyto_placeholders(G, n, own.ctypes.data, own.strides[0] // item, _PH_IN[own.dtype], short, out.ctypes.data,
                                            short, key.ctypes.data_as(u32p), ctypes.byref(pos), ctypes.byref(words), int(rbuf_bytes),
                                            device_id))
    return out, ("MT19937", key, pos.value, state[3], state[4]), words.value


def mt19937_fill(n, device_id=0):
    """The next n raw 32-bit words of numpy's global legacy stream, generated on the GPU (C ABI: cyto_mt19937_fill, the
    generator of downsample_device alone); numpy's global state is advanced past them, as
    np.random.randint(0, 2**32, n, dtype=np.uint32) would advance it."""
    state = np.random.get_state()
    key = np.array(state[1], dtype=np.uint32)
    pos = ctypes.c_int32(int(state[2]))
    out = np.empty(int(n), np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    _lib.check(_lib.lib().cyto_mt19937_fill(key.ctypes.data_as(u32p), ctypes.byref(pos), int(n), out.ctypes.data_as(u32p), device_id))
    np.random.set_state(("MT19937", key, pos.value, state[3], state[4]))
    return out


def check_paths(output_folder, output_prefix):
    """cytospace/common/common.py:176-187: the output folder (relative to the working directory) is created if needed; a
    warning is printed when results with this prefix would be overwritten.  Returns its absolute path."""
    import os
    output_path = os.path.join(os.getcwd(), output_folder)
    os.makedirs(output_path, exist_ok=True)
    if os.path.exists(os.path.join(output_path, f"{output_prefix}assigned_locations.csv")):
        print("\033[91mWARNING\033[0m: Running this will overwrite previous results, choose a new"
              " 'output_folder' or 'output_prefix'")
    return output_path


class StandardizedMatrix:
    """A gene x column matrix as the float32 GEMM operand of a metric, zero padded, resident in HBM:
    standardised values (Pearson), standardised average-tie ranks (Spearman) or the plain values (Euclidean)."""

    def __init__(self, data, already_normalized=False, device_id=0, metric="Pearson_correlation"):
        x, is64 = _as_matrix(data)
        self.G, self.C = x.shape
        self.Gpad = -(-self.G // _BK) * _BK
        self.ld = -(-self.C // _BM) * _BM
        self.device_id = device_id
        self.buf = _lib.DeviceBuffer(self.Gpad * self.ld * 4, device_id)
        _lib.check(_lib.lib().cyto_transform(METRICS[metric], self.G, self.C, x.ctypes.data, self.C, is64, 0,
                                             int(already_normalized), self.buf.ptr, self.ld, self.Gpad, device_id, None))

    def to_numpy(self):
        return self.buf.to_numpy((self.Gpad, self.ld), np.float32)[:self.G, :self.C]


def pearson_cost_device(sc_norm, st_norm, slots, device_id=0, already_normalized=True, metric="Pearson_correlation"):
    """The cost matrix of calculate_cost's lapjv branch (-Pearson, -Spearman or Euclidean distance, spots x cells)
    with every spot row repeated slots[s] times, left in HBM.

    Returns (DeviceBuffer cost, N, ld, gemm_ms).  sc_norm: G x C, st_norm: G x S."""
    sc_norm = np.asarray(sc_norm)
    st_norm = np.asarray(st_norm)
    if sc_norm.shape[0] != st_norm.shape[0]:
        raise ValueError("The two matrices v1 and v2 must have equal dimensions; "
                         "ST and scRNA data must have the same genes")
    slots = np.ascontiguousarray(slots, dtype=np.int64)
    if slots.ndim != 1 or len(slots) != st_norm.shape[1] or (slots < 0).any():
        raise ValueError("cell_number_to_node_assignment must hold one non-negative count per spot")
    if metric not in METRICS:
        raise ValueError(f"unknown distance_metric {metric!r}")
    zsc = StandardizedMatrix(sc_norm, already_normalized, device_id, metric)
    zst = StandardizedMatrix(st_norm, already_normalized, device_id, metric)
    N = int(slots.sum())
    C = zsc.C
    ld = -(-C // 4) * 4
    cost = _lib.DeviceBuffer(max(N, 1) * ld * 4, device_id)
    ms = ctypes.c_double()
    _lib.check(_lib.lib().cyto_cost_metric(METRICS[metric], zst.Gpad, zst.C, C, zst.buf.ptr, zst.ld, zsc.buf.ptr, zsc.ld,
                                           slots.ctypes.data, cost.ptr, ld, ctypes.byref(ms), device_id, None))
    zsc.buf.free()
    zst.buf.free()
    return cost, N, ld, ms.value


def matrix_correlation_pearson(v1, v2, device_id=0):
    """cytospace/common/common.py:190-199 on the GPU: corr[s, c] of column s of v2 and column c of v1.
    float32 result (standardise-then-contract on the fp32 matrix cores)."""
    v1 = np.asarray(v1)
    v2 = np.asarray(v2)
    if v1.shape[0] != v2.shape[0]:
        raise ValueError("The two matrices v1 and v2 must have equal dimensions; "
                         "ST and scRNA data must have the same genes")
    S, C = v2.shape[1], v1.shape[1]
    cost, N, ld, _ = pearson_cost_device(v1, v2, np.ones(S, np.int64), device_id, already_normalized=True)
    out = cost.to_numpy((N, ld), np.float32)[:, :C]
    cost.free()
    return -out


def matrix_correlation_spearman(v1, v2, device_id=0):
    """cytospace/common/common.py:202-215 on the GPU: Pearson correlation of the per-column average-tie ranks."""
    v1 = np.asarray(v1)
    v2 = np.asarray(v2)
    if v1.shape[0] != v2.shape[0]:
        raise ValueError("The two matrices v1 and v2 must have equal dimensions; "
                         "ST and scRNA data must have the same genes")
    S, C = v2.shape[1], v1.shape[1]
    cost, N, ld, _ = pearson_cost_device(v1, v2, np.ones(S, np.int64), device_id, True, "Spearman_correlation")
    out = cost.to_numpy((N, ld), np.float32)[:, :C]
    cost.free()
    return -out
