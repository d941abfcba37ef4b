"""CPU tests (no GPU) of the device CSV writer (csrc/csv.hip, post_processing.write_csv_device): cyto_csv_format_fields runs on the
host the one function (fmt_value) that the device's count and format passes call, and is compared byte for byte with the fields
DataFrame.to_csv writes for the same values; the header line and the gene labels, which the host formats, against pandas' own for
labels that need quoting; the C entry point's argument checks; and the fallbacks and the save_results branch that never reach the
library."""
import ctypes
import io
import os

import numpy as np
import pandas as pd
import pytest

CODES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint16): 2, np.dtype(np.uint8): 3, np.dtype(np.int32): 4,
         np.dtype(np.int64): 5}
BAD_ARG, UNSUPPORTED = 1, 7


def format_fields(values):
    """(status, the fields, the lens array) of cyto_csv_format_fields."""
    from cytospace_amd import _lib
    values = np.ascontiguousarray(values)
    n = len(values)
    out = np.zeros(20 * n + 1, np.uint8)
    lens = np.zeros(n + 1, np.int32)
    st = _lib.lib().cyto_csv_format_fields(values.ctypes.data, CODES[values.dtype], n, out.ctypes.data, 20 * n, lens.ctypes.data)
    if st:
        return st, None, lens[:n]
    assert np.all(lens[:n] > 0) and lens[:n].sum() <= 20 * n
    at = np.concatenate([[0], np.cumsum(lens[:n])])
    b = out.tobytes()
    return st, [b[at[i]:at[i + 1]] for i in range(n)], lens[:n]


def pandas_fields(values):
    """The fields DataFrame.to_csv writes for a one-column frame of `values`."""
    text = pd.DataFrame({"v": np.asarray(values)}).to_csv(index=False, header=False).encode()
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) == len(values) + 1
    return lines[:-1]


def check(values):
    values = np.asarray(values)
    st, got, _ = format_fields(values)
    assert st == 0
    want = pandas_fields(values)
    bad = [(i, values[i], got[i], want[i]) for i in range(len(values)) if got[i] != want[i]]
    assert not bad, bad[:5]
    return got


def digit_counts(limit):
    """Integers in [0, limit]: every digit count, with trailing zeros, around every power of ten and of two, and random ones."""
    rng = np.random.default_rng(3)
    vals = [0, 1, 2, 5, 9, limit, limit - 1, limit // 2, limit // 2 + 1]
    for k in range(len(str(limit))):
        vals += [v for v in (10**k - 1, 10**k, 10**k + 1, 7 * 10**k, 12 * 10**k, 1234567 * 10**k) if 0 <= v <= limit]
    for bits in range(1, limit.bit_length() + 1):
        vals += [v for v in (2**bits - 1, 2**bits, 2**bits + 1) if v <= limit]
        vals += [int(v) for v in rng.integers(1 << (bits - 1), min(limit, (1 << bits) - 1), 20, endpoint=True, dtype=np.uint64)]
    return vals


def test_int64_fields_equal_pandas_at_every_digit_count_and_the_extremes():
    vals = digit_counts(2**63 - 1)
    got = check(np.array(vals + [-v for v in vals] + [-2**63, -2**63 + 1], np.int64))
    assert max(len(g) for g in got) == 20 and b"-9223372036854775808" in got and b"9223372036854775807" in got and b"0" in got


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_narrow_integer_fields_equal_pandas(dtype):
    ii = np.iinfo(dtype)
    if dtype == np.int32:
        vals = digit_counts(ii.max)
        vals = vals + [-v for v in vals] + [ii.min, ii.min + 1]
    else:
        vals = np.arange(0, ii.max + 1)                      # every value of the type: 255 and 65535 among them
    got = check(np.array(vals, dtype))
    assert str(ii.max).encode() in got and str(ii.min).encode() in got


@pytest.mark.parametrize("dtype,limit", [(np.float32, 2**24), (np.float64, 2**53)])
def test_integer_valued_real_fields_equal_pandas_up_to_the_limit(dtype, limit):
    vals = digit_counts(limit - 1)
    a = np.array(vals + [-v for v in vals], np.int64).astype(dtype)
    assert np.array_equal(a.astype(np.int64), vals + [-v for v in vals])                  # every value is exact in dtype
    got = check(a)
    assert f"{limit - 1}.0".encode() in got and f"-{limit - 1}.0".encode() in got
    got = check(np.array([0.0, -0.0, 1.0, -1.0, 10.0, 2500.0, -100000.0], dtype))          # zeros keep their sign; trailing zeros stay
    assert got == [b"0.0", b"-0.0", b"1.0", b"-1.0", b"10.0", b"2500.0", b"-100000.0"]
    if dtype == np.float32:                                                               # ... and every integer of the last decade
        check(np.arange(2**24 - 200000, 2**24, dtype=np.int64).astype(np.float32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_real_values_outside_the_grammar_are_refused_with_their_kind(dtype):
    limit = 2.0**24 if dtype == np.float32 else 2.0**53
    big = 1e30 if dtype == np.float32 else 1e300
    for x, kind in [(0.5, 2), (-1.5, 2), (1e-30, 2), (np.nan, 3), (np.inf, 3), (-np.inf, 3), (limit, 4), (-limit, 4), (big, 4)]:
        st, _, lens = format_fields(np.array([3, x], dtype))
        assert st == UNSUPPORTED and lens[0] == 3 and lens[1] == -kind, (x, lens)


def blob_text(index_labels, column_labels, index_name):
    """The header and label bytes of csv_header_and_labels with a field b"1" per column: a whole file."""
    from cytospace_amd.post_processing import csv_header_and_labels
    header, labels, off = csv_header_and_labels(index_labels, column_labels, index_name)
    assert off.dtype == np.int64 and off[0] == 0 and off[-1] == len(labels) and len(off) == len(index_labels) + 1
    row = b",".join([b"1"] * len(column_labels)) + b"\n"
    return header + b"".join(labels[off[g]:off[g + 1]] + row for g in range(len(index_labels)))


QUOTING = ["plain", "with,comma", 'with"quote', "with\nnewline", " leading space", "", "trailing ", "gène_µ_細胞", "a'b", '"', ",", "x" * 300,
           "tab\there", "cr\rhere"]


@pytest.mark.parametrize("index_name", [None, "Gene", "a,b", ""])
def test_header_and_labels_equal_pandas(index_name):
    ones = np.ones((len(QUOTING), len(QUOTING)), np.int64)
    want = pd.DataFrame(ones, index=pd.Index(QUOTING, name=index_name), columns=QUOTING[::-1]).to_csv().encode()
    assert blob_text(QUOTING, QUOTING[::-1], index_name) == want
    # the issue's own measurement: an empty label in a row with other fields is empty, not ""
    assert blob_text([""], ["c"], None) == b",c\n,1\n" == pd.DataFrame([[1]], index=[""], columns=["c"]).to_csv().encode()
    # integer labels (a RangeIndex, numpy integers, an integer index name)
    want = pd.DataFrame(np.ones((3, 2), np.int64), index=pd.RangeIndex(5, 8, name=index_name), columns=np.array([10, -3])).to_csv().encode()
    assert blob_text(range(5, 8), np.array([10, -3]), index_name) == want
    want = pd.DataFrame(np.ones((2, 2), np.int64), index=pd.Index([1, 2], name=7), columns=["a", "b"]).to_csv().encode()
    assert blob_text([1, 2], ["a", "b"], 7) == want


def test_labels_pandas_formats_by_its_own_rules_are_not_taken():
    from cytospace_amd.post_processing import csv_header_and_labels
    for labels in ([1.5, 2.0], ["a", None], ["a", float("nan")], [("a", 1), ("b", 2)], [True, False], [pd.Timestamp("2020-01-01")]):
        assert csv_header_and_labels(labels, ["c"]) is None
        assert csv_header_and_labels(["g"] * len(labels), labels) is None
    assert csv_header_and_labels(["g"], ["c"], index_name=1.5) is None


def test_csv_write_argument_validation_needs_no_device():
    from cytospace_amd import _lib
    L = _lib.lib()
    info = _lib.CsvInfo()
    x = np.ones((2, 3), np.uint8)
    cols = np.array([0, 2], np.int64)
    off = np.array([0, 2, 4], np.int64)
    head, labels, path = b",a,b\n", b"g,h,", b"/nonexistent/new_scRNA.csv"

    def call(path=path, G=2, N=3, x=x.ctypes.data, ldx=3, dt=3, cols=cols.ctypes.data, C=2, head=head, hl=len(head), labels=labels,
             off=off.ctypes.data, bb=0, info=ctypes.byref(info)):
        return L.cyto_csv_write(path, G, N, x, ldx, dt, cols, C, head, hl, labels, off, bb, 0, info)
    for kw in (dict(path=None), dict(x=None), dict(cols=None), dict(head=None), dict(labels=None), dict(off=None), dict(info=None),
               dict(G=0), dict(G=-1), dict(N=0), dict(N=-3), dict(C=0), dict(C=-2), dict(hl=-1), dict(bb=-1), dict(ldx=2),
               dict(dt=6), dict(dt=-1), dict(dt=99),
               dict(cols=np.array([0, 3], np.int64).ctypes.data), dict(cols=np.array([-1, 1], np.int64).ctypes.data),
               dict(off=np.array([0, 3, 2], np.int64).ctypes.data), dict(off=np.array([2, 1, 4], np.int64).ctypes.data),
               dict(off=np.array([-1, 2, 4], np.int64).ctypes.data)):
        assert call(**kw) == BAD_ARG, sorted(kw)
    assert ctypes.sizeof(_lib.CsvInfo) == 56
    # the host formatter's own checks
    lens = np.zeros(2, np.int32)
    out = np.zeros(40, np.uint8)
    v = np.array([1, 2], np.int64)
    assert L.cyto_csv_format_fields(None, 5, 0, None, 0, None) == 0
    assert L.cyto_csv_format_fields(None, 5, 2, out.ctypes.data, 40, lens.ctypes.data) == BAD_ARG
    assert L.cyto_csv_format_fields(v.ctypes.data, 5, 2, out.ctypes.data, 39, lens.ctypes.data) == BAD_ARG      # room for 20 bytes each
    assert L.cyto_csv_format_fields(v.ctypes.data, 9, 2, out.ctypes.data, 40, lens.ctypes.data) == BAD_ARG
    assert L.cyto_csv_format_fields(v.ctypes.data, 5, -1, out.ctypes.data, 40, lens.ctypes.data) == BAD_ARG
    assert L.cyto_csv_format_fields(v.ctypes.data, 5, 2, out.ctypes.data, 40, lens.ctypes.data) == 0 and list(lens) == [1, 1]


def pandas_bytes(frame, columns, index_labels=None, column_labels=None, index_name=None):
    out = frame.iloc[:, columns]
    if index_labels is not None:
        out.index = index_labels
    if column_labels is not None:
        out.columns = column_labels
    if index_name is not None:
        out.index.name = index_name
    b = io.StringIO()
    out.to_csv(b, lineterminator="\n")
    return b.getvalue().encode()


def test_write_csv_device_host_side_fallbacks_need_no_device(tmp_path, monkeypatch):
    # an unknown dtype, mixed dtypes, duplicate labels, labels of other kinds and empty selections never reach the library; what was at
    # the path is gone when pandas starts
    from cytospace_amd import _lib, post_processing

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    rng = np.random.default_rng(5)
    base = rng.poisson(1.0, (4, 6))
    mixed = pd.DataFrame({"a": [1, 2, 0, 4], "b": [0.0, 2.0, 3.0, 0.0], "c": [5, 0, 0, 1]})
    cases = [("dtype uint64", pd.DataFrame(base.astype(np.uint64)), [0, 1, 5]),
             ("dtype bool", pd.DataFrame(base > 0), [0, 1, 5]),
             ("dtype uint32", pd.DataFrame(base.astype(np.uint32)), [0, 1, 5]),
             ("dtype object", pd.DataFrame(base.astype(object)), [0, 1, 5]),
             ("duplicate labels", pd.DataFrame(base, columns=list("abcdea")), [0, 1, 2]),
             ("mixed dtypes", mixed, [0, 1, 1]),
             ("labels", pd.DataFrame(base, index=[0.5, 1.5, 2.5, 3.5]), [3, 3]),
             ("empty", pd.DataFrame(base), []),
             ("empty", pd.DataFrame(base[:0]), [1, 2])]
    p = str(tmp_path / "t.csv")
    seen = []
    real = pd.DataFrame.to_csv

    def watched(self, target=None, *a, **kw):
        seen.append(os.path.exists(p))
        return real(self, target, *a, **kw)
    monkeypatch.setattr(pd.DataFrame, "to_csv", watched)
    for reason, m, cols in cases:
        open(p, "wb").write(b"stale")
        info = post_processing.write_csv_device(p, m, cols, return_info=True)
        assert info["path"] == "pandas" and info["reason"] == reason, (reason, info)
        assert seen[-1] is False, reason
        assert open(p, "rb").read() == pandas_bytes(m, cols), reason
    buf = io.StringIO()
    info = post_processing.write_csv_device(buf, pd.DataFrame(base), [1, 0], return_info=True)
    assert info["reason"] == "not a path" and buf.getvalue().encode() == pandas_bytes(pd.DataFrame(base), [1, 0])
    # an array takes range labels; the given labels and name replace a frame's own
    post_processing.write_csv_device(p, base.astype(np.uint64), [5, -1])
    assert open(p, "rb").read() == pandas_bytes(pd.DataFrame(base), [5, 5], column_labels=[5, 5])
    post_processing.write_csv_device(p, pd.DataFrame(base > 0), [2, 0], index_labels=list("wxyz"), column_labels=["p", "q"], index_name="n")
    assert open(p, "rb").read() == pandas_bytes(pd.DataFrame(base > 0), [2, 0], list("wxyz"), ["p", "q"], "n")
    os.remove(p)
    with pytest.raises(IndexError):
        post_processing.write_csv_device(p, base, [0, 6])
    with pytest.raises(ValueError):
        post_processing.write_csv_device(p, base, [0, 1], column_labels=["a"])
    assert not os.path.exists(p)


def _toy():
    rng = np.random.default_rng(12)
    G, C, S = 7, 14, 6
    cells = [f"CELL_c{i}" for i in range(C)]
    ctd = pd.DataFrame({"CellType": [["TYPE_B", "TYPE_T", "TYPE_Mono"][i % 3] for i in range(C)]}, index=cells)
    expr = pd.DataFrame(rng.poisson(2.0, (G, C)), index=[f"GENE_g{i}" for i in range(G)], columns=cells)
    for k, t in enumerate(["B", "Mono"]):
        expr[f"CELL_{t}_new_{k + 1}"] = rng.poisson(2.0, G)
    coords = pd.DataFrame({"row": np.arange(S) // 3, "col": np.arange(S) % 3}, index=[f"SPOT_s{i}" for i in range(S)])
    picked = [cells[i] for i in (3, 0, 7, 7, 12, 5, 9, 1, 3)] + list(expr.columns[-2:])
    spots = [coords.index[i] for i in (0, 0, 1, 3, 3, 3, 4, 1, 0, 4, 3)]
    return picked, expr, coords.loc[spots], ctd


def _files(d):
    return {os.path.relpath(os.path.join(r, f), str(d)): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(str(d)) for f in fs}


def test_save_results_place_holders_without_a_device_never_touches_the_writer(tmp_path, monkeypatch):
    from cytospace_amd import _lib, post_processing

    def no_library(*a, **k):
        raise AssertionError("save_results(device_id=None) went to the device writer")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(post_processing, "write_csv_device", no_library)
    picked, expr, assigned, ctd = _toy()
    post_processing.save_results(str(tmp_path), "p_", np.array(picked), expr, assigned, ctd, "place_holders", False)
    assert _files(tmp_path)["p_new_scRNA.csv"].startswith(b",B_new_1,Mono_new_2\ng0,")
    # non-unique columns keep the host code too, whatever the device
    twice = pd.concat([expr, expr.iloc[:, -1:]], axis=1)
    (tmp_path / "b").mkdir()
    post_processing.save_results(str(tmp_path / "b"), "p_", np.array(picked), twice, assigned, ctd, "place_holders", False, device_id=0)
    assert _files(tmp_path / "b")["p_new_scRNA.csv"].startswith(b",B_new_1,Mono_new_2,Mono_new_2\ng0,")


def test_save_results_place_holders_with_a_device_hands_positions_and_stripped_labels_to_the_writer(tmp_path, monkeypatch):
    # the writer is replaced by pandas on what it was given (no device): the same files as the host branch
    from cytospace_amd import post_processing
    calls = []

    def stand_in(path, frame, columns, index_labels=None, column_labels=None, index_name=None, device_id=0, **kw):
        calls.append((list(columns), list(column_labels), device_id))
        open(path, "wb").write(pandas_bytes(frame, list(columns), index_labels, column_labels, index_name))
    monkeypatch.setattr(post_processing, "write_csv_device", stand_in)
    picked, expr, assigned, ctd = _toy()
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    post_processing.save_results(str(tmp_path / "a"), "p_", np.array(picked), expr, assigned, ctd, "place_holders", False)
    assert calls == []
    post_processing.save_results(str(tmp_path / "b"), "p_", np.array(picked), expr, assigned, ctd, "place_holders", False, device_id=3)
    assert calls == [([14, 15], ["B_new_1", "Mono_new_2"], 3)]
    assert _files(tmp_path / "a") == _files(tmp_path / "b") and "p_new_scRNA.csv" in _files(tmp_path / "a")


def test_save_results_place_holders_drops_the_index_name_on_both_branches(tmp_path, monkeypatch):
    # a frame whose index has a name (read_file's frames have one): the host branch's list of labels drops it, and the device branch
    # asks the writer for no name -- also when the writer hands the frame on to pandas (a uint64 frame never reaches the library)
    from cytospace_amd import _lib, post_processing

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    picked, expr, assigned, ctd = _toy()
    expr = expr.astype(np.uint64)
    expr.index.name = "GENES"
    got = {}
    for tag, dev in (("host", None), ("device", 0)):
        (tmp_path / tag).mkdir()
        post_processing.save_results(str(tmp_path / tag), "p_", np.array(picked), expr, assigned, ctd, "place_holders", False, device_id=dev)
        got[tag] = _files(tmp_path / tag)
    assert got["host"] == got["device"] and got["host"]["p_new_scRNA.csv"].startswith(b",B_new_1,Mono_new_2\ng0,")
    assert expr.index.name == "GENES"
    # ... and the stand-in writer of the test above is handed index_name="" for such a frame
    seen = []
    monkeypatch.setattr(post_processing, "write_csv_device", lambda path, frame, columns, **kw: seen.append(kw["index_name"]))
    (tmp_path / "c").mkdir()
    post_processing.save_results(str(tmp_path / "c"), "p_", np.array(picked), expr, assigned, ctd, "place_holders", False, device_id=1)
    assert seen == [""]
