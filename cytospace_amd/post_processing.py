"""Output writers of the reference: `save_results`
(/root/reference/cytospace/post_processing/post_processing.py:10-116) and the unassigned-spot table written by
main_cytospace (/root/reference/cytospace/cytospace.py:686-694).  Host code (pandas), same file names, columns and
ordering, so a run of this package can be post-processed by the same downstream scripts; with a device, the one large file of a run
(assigned_expression/matrix.mtx, or new_scRNA.csv with place-holders) is formatted on the GPU by write_mtx_device / write_csv_device,
byte for byte what scipy / pandas writes.  Written from the format, not from the reference's statements: tests/golden/gv12_* holds
files the reference itself wrote for the same inputs.
"""
import math
import os

import numpy as np
import pandas as pd

from . import _lib


def _strip(prefix, names):
    n = len(prefix)
    return [str(x)[n:] for x in names]          # the reference drops the first five characters ('CELL_', 'SPOT_', ...)


def assigned_locations_table(cell_ids_selected, assigned_locations, cell_type_data, sampling_method):
    """The rows of <prefix>assigned_locations.csv: one per assigned cell, in assignment order.
    UniqueCID = 'UCID' + zero-padded running number (width = digits of the cell count); a cell that is not in
    cell_type_data is a place-holder: OriginalCID 'NA', its type read from its id 'CELL_<type>_new_<k>'."""
    ids = [str(c) for c in cell_ids_selected]
    width = int(math.log10(len(ids))) + 1
    known = set(cell_type_data.index)
    type_col = cell_type_data.columns[0]
    cols = {"UniqueCID": ["UCID" + str(i).zfill(width) for i in range(len(ids))],
            "OriginalCID": _strip("CELL_", [c if c in known else "CELL_NA" for c in ids])}
    if sampling_method == "place_holders":
        cols["PlaceHolderCID"] = _strip("CELL_", ids)
    cols["CellType"] = _strip("TYPE_", [cell_type_data.at[c, type_col] if c in known else "TYPE_" + c.split("_")[1] for c in ids])
    cols["SpotID"] = _strip("SPOT_", assigned_locations.index)
    for k in range(2):
        cols[assigned_locations.columns.values[k]] = list(assigned_locations.iloc[:, k])
    return pd.DataFrame.from_dict(cols)


# numpy dtype -> (the dtype uploaded, CYTO_DTYPE_*) of write_mtx_device; every other dtype is written by scipy
_MTX_DTYPES = {"uint8": (np.uint8, _lib.CYTO_DTYPE_U8), "uint16": (np.uint16, _lib.CYTO_DTYPE_U16), "int8": (np.int32, _lib.CYTO_DTYPE_I32),
               "int16": (np.int32, _lib.CYTO_DTYPE_I32), "int32": (np.int32, _lib.CYTO_DTYPE_I32), "int64": (np.int64, _lib.CYTO_DTYPE_I64),
               "float32": (np.float32, _lib.CYTO_DTYPE_F32), "float64": (np.float64, _lib.CYTO_DTYPE_F64)}
_MTX_REFUSALS = {_lib.CYTO_MTX_ERR_FRACTION: "non-integer value", _lib.CYTO_MTX_ERR_NONFINITE: "non-finite value",
                 _lib.CYTO_MTX_ERR_MAGNITUDE: "magnitude", _lib.CYTO_MTX_ERR_SQUARE: "square", _lib.CYTO_MTX_ERR_IO: "io"}


def _mtx_narrow(x, fractions=False):
    """x (one of _MTX_DTYPES) as the narrowest array the device formats to the same text, and its CYTO_DTYPE_*.  Integers: the
    field stays "integer" (uint8 / uint16 / int32 / int64 by range).  float64: float32 when every value is one and lies below 2^24,
    where both types' shortest digits are the integer's own.  fractions: the device then writes a float32 that is no integer by
    float32's shortest digits (0.1 for the float64 0.10000000149011612), so every value must be an integer as well."""
    to, code = _MTX_DTYPES[x.dtype.name]
    if x.dtype.kind in "iu" and x.size:
        lo, hi = int(x.min()), int(x.max())
        if lo >= 0 and hi < (1 << 8):
            to, code = np.uint8, _lib.CYTO_DTYPE_U8
        elif lo >= 0 and hi < (1 << 16):
            to, code = np.uint16, _lib.CYTO_DTYPE_U16
        elif -(1 << 31) <= lo and hi < (1 << 31):
            to, code = np.int32, _lib.CYTO_DTYPE_I32
    elif x.dtype == np.float64 and x.size:
        if -(1 << 24) < x.min() and x.max() < (1 << 24):     # (False with a NaN: the device refuses it whatever the type)
            x32 = x.astype(np.float32)
            step = max(1, (1 << 24) // x.shape[1])           # (compared in row blocks: array_equal widens its block to float64)
            if all(np.array_equal(x32[r:r + step], x[r:r + step]) and
                   (not fractions or np.array_equal(np.trunc(x32[r:r + step]), x32[r:r + step]))
                   for r in range(0, x.shape[0], step)):
                return np.ascontiguousarray(x32), _lib.CYTO_DTYPE_F32
    return np.ascontiguousarray(x, dtype=to), code


def write_mtx_device(path, matrix_or_frame, columns, device_id=0, block_bytes=0, return_info=False, fractions=False):
    """scipy.io.mmwrite(path, scipy.sparse.coo_matrix(frame.iloc[:, columns])) with the text formatted on the GPU (C ABI:
    cyto_mtx_write; csrc/mtx.hip): the same bytes.  matrix_or_frame: genes x cells, a DataFrame or a 2-D array; columns: the
    positions (not labels) of the cells to write, in file order, repeats allowed.  block_bytes: the most text per device buffer
    (0: the library's default; tests force many blocks with it).

    What the device does not format is written by scipy itself: a real matrix with a non-zero that is not an
    integer below 2^53 (2^24 for float32), a square result, a dtype other than int8..int64 / uint8 / uint16 / float32 / float64,
    a frame whose column labels are not unique or whose selected columns have another common dtype than the whole frame, an empty
    result, a path that is not a str.

    fractions=True (C ABI: cyto_mtx_write_ex with CYTO_TEXT_FRACTIONS; save_results passes it): the device writes every finite real
    value, by the shortest digits that read back as the same value of the matrix's dtype, as scipy does ("1E-1", "2.5",
    "3.333333333333333E-1", "5E-324"); of the real values only NaN and +-inf ("non-finite value") still go to scipy.

    matrix_or_frame may be a resident.DeviceFrame: the values are read where they lie in HBM (C ABI: cyto_mtx_write_dev; a frame
    that is a view of some of its buffer's rows is gathered on the device first), the same bytes; what the device refuses -- a
    square result, a non-finite value -- is written by scipy from the fetched frame (noted in resident.last_run["fallbacks"]).

    return_info: also return a dict -- "path" ("device" or "scipy"), for a fallback "reason", and for the device "nnz", "bytes",
    "field", "blocks" and the phase times in seconds: narrow_s (the host's choice of the upload dtype), library_s (the whole
    cyto_mtx_write call: device and pinned allocations and their release besides the next four), upload_s, kernels_s, download_s
    (overlaps the others), write_s, total_s."""
    import ctypes
    import time
    import pandas as pd
    import scipy.io
    import scipy.sparse
    t0 = time.perf_counter()
    info = {"path": "device"}
    from . import resident as _resident
    dframe = matrix_or_frame if _resident.is_frame(matrix_or_frame) else None
    frame = matrix_or_frame if isinstance(matrix_or_frame, pd.DataFrame) else None
    if frame is None and dframe is None:
        matrix_or_frame = np.asarray(matrix_or_frame)
        if matrix_or_frame.ndim != 2:
            raise ValueError("write_mtx_device needs a 2-D matrix")
    G, N = matrix_or_frame.shape
    columns = np.asarray(columns, dtype=np.int64).reshape(-1)
    if columns.size and (columns.min() < -N or columns.max() >= N):
        raise IndexError("positional indexers are out-of-bounds")
    columns = np.ascontiguousarray(np.where(columns < 0, columns + N, columns))
    C = len(columns)

    def selected():
        if dframe is not None:
            return dframe.take(cols=columns).to_frame()
        return frame.iloc[:, columns] if frame is not None else matrix_or_frame[:, columns]

    def refuse(reason):
        if dframe is not None:
            _resident.record_fallback("write_mtx", reason)
        info.update(path="scipy", reason=reason)
        scipy.io.mmwrite(path, scipy.sparse.coo_matrix(selected()))
        info["total_s"] = time.perf_counter() - t0
        return info if return_info else None

    if not isinstance(path, str):
        return refuse("not a path")
    if G == 0 or C == 0:
        return refuse("empty")
    if G == C:
        return refuse("square")
    if dframe is not None:
        if not dframe.columns.is_unique:
            return refuse("duplicate labels")
        # the buffer itself when the view keeps every row (the column positions go through the view's own); else one gather
        rows, cols = dframe.positions
        mat = dframe if rows is None else dframe.take(cols=columns).materialize()
        try:
            if rows is not None:
                src, N0 = np.arange(C, dtype=np.int64), C
            else:
                src, N0 = np.ascontiguousarray(columns if cols is None else cols[columns]), dframe.buffer_shape[1]
            mi = _lib.MtxInfo()
            t = time.perf_counter()
            st = _lib.lib().cyto_mtx_write_dev(path.encode(), G, N0, mat.ptr, mat.ld, mat.code, src.ctypes.data, C, int(block_bytes),
                                               device_id, _lib.CYTO_TEXT_FRACTIONS if fractions else 0, ctypes.byref(mi))
            info["library_s"] = time.perf_counter() - t
        finally:
            if mat is not dframe:
                mat.close()
        if st == _lib.CYTO_ERR_UNSUPPORTED:                                  # nothing is left at `path`
            return refuse(_MTX_REFUSALS.get(mi.reason, str(mi.reason)))
        _lib.check(st)
        info.update(nnz=mi.nnz, bytes=mi.bytes, field="real" if mi.field else "integer", blocks=mi.blocks, upload_s=mi.ms_upload / 1e3,
                    kernels_s=mi.ms_kernels / 1e3, download_s=mi.ms_download / 1e3, write_s=mi.ms_write / 1e3)
        info["total_s"] = time.perf_counter() - t0
        return info if return_info else None
    if frame is not None:
        if not frame.columns.is_unique:
            return refuse("duplicate labels")
        kinds = frame.dtypes.unique()
        if len(kinds) > 1 and frame.iloc[:0, columns].to_numpy().dtype != frame.iloc[:0].to_numpy().dtype:
            return refuse("mixed dtypes")
    x = frame.to_numpy() if frame is not None else matrix_or_frame
    if x.dtype.name not in _MTX_DTYPES:
        return refuse(f"dtype {x.dtype}")
    t = time.perf_counter()
    x, code = _mtx_narrow(x, fractions)
    info["narrow_s"] = time.perf_counter() - t
    mi = _lib.MtxInfo()
    t = time.perf_counter()
    if fractions:
        st = _lib.lib().cyto_mtx_write_ex(path.encode(), G, N, x.ctypes.data, N, code, columns.ctypes.data, C, int(block_bytes),
                                          device_id, _lib.CYTO_TEXT_FRACTIONS, ctypes.byref(mi))
    else:
        st = _lib.lib().cyto_mtx_write(path.encode(), G, N, x.ctypes.data, N, code, columns.ctypes.data, C, int(block_bytes), device_id,
                                       ctypes.byref(mi))
    info["library_s"] = time.perf_counter() - t
    if st == _lib.CYTO_ERR_UNSUPPORTED:                                      # nothing is left at `path`
        return refuse(_MTX_REFUSALS.get(mi.reason, str(mi.reason)))
    _lib.check(st)
    info.update(nnz=mi.nnz, bytes=mi.bytes, field="real" if mi.field else "integer", blocks=mi.blocks, upload_s=mi.ms_upload / 1e3,
                kernels_s=mi.ms_kernels / 1e3, download_s=mi.ms_download / 1e3, write_s=mi.ms_write / 1e3)
    info["total_s"] = time.perf_counter() - t0
    return info if return_info else None


# numpy dtype -> (the dtype uploaded, CYTO_DTYPE_*) of write_csv_device; every other dtype is written by pandas.  No narrowing here:
# the text depends on the dtype's kind alone, and choosing a narrower upload would be a host pass over the matrix.
_CSV_DTYPES = _MTX_DTYPES
_CSV_REFUSALS = {_lib.CYTO_CSV_ERR_FRACTION: "non-integer value", _lib.CYTO_CSV_ERR_NONFINITE: "non-finite value",
                 _lib.CYTO_CSV_ERR_MAGNITUDE: "magnitude", _lib.CYTO_CSV_ERR_IO: "io"}


class _Rows(list):
    """The file object of a csv.writer that keeps each row's text apart (the writer calls write() once per row)."""
    write = list.append


def _csv_labels(labels):
    """labels as the strings csv.writer gets from pandas, or None: strings stay, integers are their digits; whatever pandas formats
    by rules of its own (floats, dates, missing values, tuples of a MultiIndex) is not taken."""
    out = []
    for v in labels:
        if isinstance(v, str):
            out.append(v)
        elif isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
            out.append(str(int(v)))
        else:
            return None
    return out


def csv_header_and_labels(index_labels, column_labels, index_name=None):
    """What the host formats of DataFrame.to_csv's text, by pandas' own means (csv.writer, QUOTE_MINIMAL, '\\n' line ends):
    (the header line, the genes' labels each with its trailing ',' as one bytes object, int64 offsets [G + 1] into it); None when a
    label is neither a string nor an integer.  An empty label stays empty: pandas quotes it only in a row without other fields."""
    import csv
    rows, cols = _csv_labels(index_labels), _csv_labels(column_labels)
    name = "" if index_name is None else _csv_labels([index_name])
    if rows is None or cols is None or name is None:
        return None
    sink = _Rows()
    w = csv.writer(sink, lineterminator="\n", delimiter=",", quoting=csv.QUOTE_MINIMAL, doublequote=True, escapechar=None, quotechar='"')
    w.writerow([name if name == "" else name[0]] + cols)
    header = sink.pop().encode("utf-8")
    w.writerows((r, "") for r in rows)                    # "<label>,\n": the second, empty field keeps an empty label unquoted
    parts = [t[:-1].encode("utf-8") for t in sink]
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    return header, b"".join(parts), off


def write_csv_device(path, matrix_or_frame, columns, index_labels=None, column_labels=None, index_name=None, device_id=0, block_bytes=0,
                     return_info=False, fractions=False):
    """out = frame.iloc[:, columns]; out.index = index_labels; out.columns = column_labels; out.index.name = index_name;
    out.to_csv(path) -- with the value fields formatted on the GPU (C ABI: cyto_csv_write; csrc/csv.hip): the same bytes, and the
    selected genes x cells frame is never built on the host.  matrix_or_frame: genes x cells, a DataFrame or a 2-D array; columns:
    the positions (not labels) of the cells to write, in file order, repeats and negative positions allowed.  index_labels (G),
    column_labels (len(columns)) and index_name default to the frame's own (an array: range(...) labels, no name); index_name=""
    writes no name where the frame has one (pandas' header is the same for "" and for None).  block_bytes: the
    most text per slab of genes (0: the library's default; tests force many slabs with it).

    The host formats the header line and the gene labels (pandas' quoting applies to them), the device every value: integer dtypes
    as decimals, float32 / float64 integers as "<digits>.0" ("-0.0" for a negative zero).  What the device does not format is
    written by pandas itself (DESIGN.md 4.1d'), after whatever was at `path` has been removed: a real value that is not an integer
    below 2^53 (2^24 for float32) -- found by the device while it counts, also in a late slab --, a dtype other than int8..int64 /
    uint8 / uint16 / float32 / float64, selected columns of more than one dtype, duplicate column labels in the source frame, labels
    that are neither strings nor integers, an empty result, a path that is not a str, a file that cannot be created or written.

    fractions=True (C ABI: cyto_csv_write_ex with CYTO_TEXT_FRACTIONS; save_results passes it): the device writes every finite real
    value as pandas does, a float64 as repr(float) ("0.0001", "0.3333333333333333", "1e-05", "1.5e+20"), a float32 by float32's own
    shortest digits in numpy's form ("0.33333334", "1e-04", "1.2345679e+17"); of the real values only NaN and +-inf ("non-finite
    value") still go to pandas.

    return_info: also return a dict -- "path" ("device" or "pandas"), for a fallback "reason", and for the device "bytes", "blocks"
    and the phase times in seconds: labels_s (the host's header and labels), library_s (the whole cyto_csv_write call: device and
    pinned allocations and their release besides the next four), upload_s, kernels_s, download_s (the three are device times and
    overlap write_s), write_s, total_s."""
    import ctypes
    import time
    t0 = time.perf_counter()
    info = {"path": "device"}
    frame = matrix_or_frame if isinstance(matrix_or_frame, pd.DataFrame) else None
    if frame is None:
        matrix_or_frame = np.asarray(matrix_or_frame)
        if matrix_or_frame.ndim != 2:
            raise ValueError("write_csv_device needs a 2-D matrix")
    G, N = matrix_or_frame.shape
    columns = np.asarray(columns, dtype=np.int64).reshape(-1)
    if columns.size and (columns.min() < -N or columns.max() >= N):
        raise IndexError("positional indexers are out-of-bounds")
    columns = np.ascontiguousarray(np.where(columns < 0, columns + N, columns))
    C = len(columns)
    if index_labels is None:
        index_labels = frame.index if frame is not None else range(G)
    if column_labels is None:
        column_labels = frame.columns[columns] if frame is not None else columns
    if index_name is None and frame is not None:
        index_name = frame.index.name
    if len(index_labels) != G or len(column_labels) != C:
        raise ValueError("write_csv_device: index_labels / column_labels do not fit the selection")

    def refuse(reason):
        info.update(path="pandas", reason=reason)
        if isinstance(path, str) and os.path.lexists(path) and not os.path.isdir(path):
            os.remove(path)
        out = frame.iloc[:, columns] if frame is not None else pd.DataFrame(matrix_or_frame[:, columns])
        out.index = pd.Index(index_labels).rename(index_name)
        out.columns = column_labels
        out.to_csv(path)
        info["total_s"] = time.perf_counter() - t0
        return info if return_info else None

    if not isinstance(path, str):
        return refuse("not a path")
    if G == 0 or C == 0:
        return refuse("empty")
    x, picked = matrix_or_frame, columns
    if frame is not None:
        if not frame.columns.is_unique:
            return refuse("duplicate labels")
        if len(frame.dtypes.unique()) > 1:                   # pandas formats each column by its own dtype ("1,1.0")
            used = np.unique(columns)
            if len(frame.dtypes.iloc[used].unique()) > 1:
                return refuse("mixed dtypes")
            x, picked = frame.iloc[:, used], np.ascontiguousarray(np.searchsorted(used, columns))
            N = len(used)
        if str(x.dtypes.iloc[0]) not in _CSV_DTYPES:         # (before to_numpy: a sparse or extension dtype is not made dense)
            return refuse(f"dtype {x.dtypes.iloc[0]}")
        x = x.to_numpy()
    if x.dtype.name not in _CSV_DTYPES:
        return refuse(f"dtype {x.dtype}")
    t = time.perf_counter()
    text = csv_header_and_labels(index_labels, column_labels, index_name)
    info["labels_s"] = time.perf_counter() - t
    if text is None:
        return refuse("labels")
    header, labels, off = text
    to, code = _CSV_DTYPES[x.dtype.name]
    x = np.ascontiguousarray(x, dtype=to)                    # (a copy for int8 / int16 and for a frame held column-major)
    ci = _lib.CsvInfo()
    t = time.perf_counter()
    if fractions:
        st = _lib.lib().cyto_csv_write_ex(path.encode(), G, N, x.ctypes.data, N, code, picked.ctypes.data, C, header, len(header), labels,
                                          off.ctypes.data, int(block_bytes), device_id, _lib.CYTO_TEXT_FRACTIONS, ctypes.byref(ci))
    else:
        st = _lib.lib().cyto_csv_write(path.encode(), G, N, x.ctypes.data, N, code, picked.ctypes.data, C, header, len(header), labels,
                                       off.ctypes.data, int(block_bytes), device_id, ctypes.byref(ci))
    info["library_s"] = time.perf_counter() - t
    if st == _lib.CYTO_ERR_UNSUPPORTED:                                      # nothing is left at `path`
        return refuse(_CSV_REFUSALS.get(ci.reason, str(ci.reason)))
    _lib.check(st)
    info.update(bytes=ci.bytes, blocks=ci.blocks, upload_s=ci.ms_upload / 1e3, kernels_s=ci.ms_kernels / 1e3,
                download_s=ci.ms_download / 1e3, write_s=ci.ms_write / 1e3)
    info["total_s"] = time.perf_counter() - t0
    return info if return_info else None


def save_results(output_path, output_prefix, cell_ids_selected, all_cells_save, assigned_locations,
                 cell_type_data, sampling_method, single_cell, device_id=None):
    """post_processing.py:10-116, same arguments, and device_id: None writes matrix.mtx / new_scRNA.csv on the host (scipy / pandas);
    a device number has write_mtx_device / write_csv_device write them (the same bytes, fractional values included).  Writes
      <prefix>assigned_locations.csv
      <prefix>assigned_expression/{genes.tsv, barcodes.tsv, matrix.mtx}     (sampling_method "duplicates")
      <prefix>new_scRNA.csv                                                 ("place_holders": the generated cells)
      <prefix>cell_type_assignments_by_spot.csv, <prefix>fractional_abundances_by_spot.csv   (not in single-cell mode)"""
    import scipy.io
    import scipy.sparse
    from . import resident as _resident
    if _resident.is_frame(all_cells_save) and (device_id is None or sampling_method != "duplicates"):
        all_cells_save = all_cells_save.to_frame()
    df = assigned_locations_table(cell_ids_selected, assigned_locations, cell_type_data, sampling_method)
    df.to_csv(os.path.join(output_path, f"{output_prefix}assigned_locations.csv"), index=False)

    if sampling_method == "duplicates":
        out_dir = os.path.join(output_path, f"{output_prefix}assigned_expression")
        if os.path.exists(out_dir):
            print("\033[91mWARNING\033[0m: {} exists and the expression matrix may be overwritten.".format(out_dir))
        os.makedirs(out_dir, exist_ok=True)
        labels = ["CELL_{}".format(x) for x in df.OriginalCID]
        positions = None
        if device_id is not None and all_cells_save.columns.is_unique:
            positions = all_cells_save.columns.get_indexer(labels)
            if (positions < 0).any():                     # (a missing label: the host path raises its KeyError)
                positions = None
        if positions is None:
            if _resident.is_frame(all_cells_save):
                _resident.record_fallback("save_results", "labels")
                all_cells_save = all_cells_save.to_frame()
            expr = all_cells_save.loc[:, labels]
            expr.index = _strip("GENE_", expr.index)
            expr.columns = df.UniqueCID
            genes = expr.index.to_frame()
            genes.reset_index(inplace=True)           # gene id twice: Read10X expects the name in the second column
            genes.to_csv(os.path.join(out_dir, "genes.tsv"), sep="\t", header=False, index=False)
            expr.columns.to_frame().to_csv(os.path.join(out_dir, "barcodes.tsv"), sep="\t", header=False, index=False)
            scipy.io.mmwrite(os.path.join(out_dir, "matrix.mtx"), scipy.sparse.coo_matrix(expr))
        else:                                         # the same three files without the gathered genes x cells frame
            genes = pd.Index(_strip("GENE_", all_cells_save.index)).to_frame()
            genes.reset_index(inplace=True)
            genes.to_csv(os.path.join(out_dir, "genes.tsv"), sep="\t", header=False, index=False)
            pd.Index(df.UniqueCID).to_frame().to_csv(os.path.join(out_dir, "barcodes.tsv"), sep="\t", header=False, index=False)
            write_mtx_device(os.path.join(out_dir, "matrix.mtx"), all_cells_save, positions, device_id=device_id, fractions=True)
    elif device_id is not None and all_cells_save.columns.is_unique:
        positions = np.flatnonzero(~all_cells_save.columns.isin(cell_type_data.index))     # the generated cells, without their frame
        write_csv_device(os.path.join(output_path, f"{output_prefix}new_scRNA.csv"), all_cells_save, positions,
                         index_labels=_strip("GENE_", all_cells_save.index.astype(str)),
                         column_labels=_strip("CELL_", all_cells_save.columns[positions].astype(str)), index_name="",
                         device_id=device_id, fractions=True)   # (the host branch's list of labels drops the index's name: none here either)
    else:
        generated = all_cells_save.loc[:, ~all_cells_save.columns.isin(cell_type_data.index)]
        generated.index = _strip("GENE_", generated.index.astype(str))
        generated.columns = _strip("CELL_", generated.columns.astype(str))
        generated.to_csv(os.path.join(output_path, f"{output_prefix}new_scRNA.csv"))

    if not single_cell:
        # SpotID x CellType counts, spots and types in order of first appearance, plus the row total
        counts = df.loc[:, ["SpotID", "CellType"]].value_counts().unstack(fill_value=0) \
            .reindex(index=df.SpotID.unique(), columns=df.CellType.unique())
        counts["Total cells"] = counts.sum(axis=1)
        counts = counts.astype(int)
        counts.index.name = "SpotID"
        counts.to_csv(os.path.join(output_path, f"{output_prefix}cell_type_assignments_by_spot.csv"))
        totals = np.array(counts["Total cells"], dtype=float)
        counts.iloc[:, :-1].div(totals, axis=0).to_csv(os.path.join(output_path, f"{output_prefix}fractional_abundances_by_spot.csv"))


def save_unassigned_locations(output_path, output_prefix, all_spot_ids, assigned_locations, coordinates_data):
    """cytospace.py:686-694: the spots that received no cell, with a 'Number of cells' column of zeros.
    Returns the number of such spots (the file is only written when there are any)."""
    unmapped = np.setdiff1d(list(all_spot_ids), list(assigned_locations.index)).tolist()
    if unmapped:
        table = coordinates_data.loc[unmapped].copy()
        table.index = table.index.str.replace("SPOT_", "")
        table["Number of cells"] = 0
        table.to_csv(f"{output_path}/{output_prefix}unassigned_locations.csv", index=True)
    return len(unmapped)
