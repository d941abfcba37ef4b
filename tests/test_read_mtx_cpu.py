"""The device MatrixMarket reader's safety rule, without a GPU: whatever the grammar accepts, read_file reads to the same bits.

The entry-line parser the kernel runs is compiled for the host too (C ABI: cyto_mtx_parse_entries).  Here it is held to
scipy.io.mmread on 10^5 value tokens of each field, the window's edges included; the header parser is tried on every banner form;
tools/mtx_read_model.py (a plain model of cyto_mtx_read) must refuse every generated file with the (kind, line, byte) its
generator planted, and for every file it accepts its words go through common._mtx_frame -- the code that builds the user's
DataFrame -- and must be equal to read_file(path, keep_sparse=False).  tests/test_read_mtx_gpu.py then holds the kernels to
read_file on the same files."""
import ctypes
import gzip
import io

import numpy as np
import pandas as pd
import pytest
import scipy.io

from tools import mtx_read_model as mm

CASES = mm.cases()
TOKEN, INEXACT, NEGZERO = 8, 9, 10


def _equal(a, b):
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    for c in range(a.shape[1]):
        x, y = a.iloc[:, c].to_numpy(), b.iloc[:, c].to_numpy()
        assert x.dtype == y.dtype
        if x.dtype == np.float64:
            assert np.array_equal(x.view(np.int64), y.view(np.int64))


def _values(tokens, field):
    """(kind, value words) of the hook for the value tokens, each in a line `1 <i> <token>`."""
    from cytospace_amd.common import parse_mtx_entries
    n = len(tokens)
    kind, _, row, col, val = parse_mtx_entries([f"1 {i + 1} {t}".encode() for i, t in enumerate(tokens)], field, 1, n)
    ok = kind == 0
    assert np.all(row[ok] == 1) and np.array_equal(col[ok], np.arange(1, n + 1)[ok])
    return kind, val


def _mmread_row(tokens, keep, field):
    """scipy's dense row for the kept tokens, one entry each."""
    name = "integer" if field == 0 else "real"
    cols = np.flatnonzero(keep)
    text = f"%%MatrixMarket matrix coordinate {name} general\n1 {len(tokens)} {len(cols)}\n" + \
        "".join(f"1 {i + 1} {tokens[i]}\n" for i in cols)
    m = scipy.io.mmread(io.BytesIO(text.encode()))
    assert m.dtype == (np.int64 if field == 0 else np.float64)
    return m.toarray()[0]


def test_real_tokens_are_scipys_values_bit_for_bit():
    tokens = mm.real_tokens(np.random.default_rng(11), 100000)
    kind, val = _values(tokens, 1)
    keep = kind == 0
    assert keep.mean() > 0.5 and set(np.unique(kind)) == {0, TOKEN, INEXACT, NEGZERO}
    want = _mmread_row(tokens, keep, 1)
    assert np.array_equal(val[keep], want.view(np.int64)[keep])
    assert not (np.signbit(want[keep]) & (want[keep] == 0)).any()                # no -0.0 got through


def test_integer_tokens_are_scipys_values():
    tokens = mm.int_tokens(np.random.default_rng(12), 100000)
    kind, val = _values(tokens, 0)
    keep = kind == 0
    assert keep.mean() > 0.5 and set(np.unique(kind)) == {0, TOKEN}
    assert np.array_equal(val[keep], _mmread_row(tokens, keep, 0)[keep])
    assert all(len(t.lstrip("-")) > 18 for t, k in zip(tokens[len(mm.EDGE_INT):], kind[len(mm.EDGE_INT):]) if k)


@pytest.mark.parametrize("token,kind", [
    ("999999999999999", 0), ("1000000000000000", INEXACT), ("9999999999999999", INEXACT), ("0.999999999999999", 0),
    ("0.9999999999999999", INEXACT), ("1e22", 0), ("1e23", INEXACT), ("1e-22", 0), ("1e-23", INEXACT), ("15e22", 0), ("15e23", INEXACT),
    ("1.5e23", 0), ("123456789012345e22", 0), ("123456789012345e-22", 0), ("1.23456789012345e-8", 0), ("1.23456789012345e-9", INEXACT),
    ("5.", 0), (".5", 0), ("5.000", 0), ("100.000e20", 0), ("1.50000000000000000000000", 0), ("000000000000000000005", 0),
    ("0", 0), ("0.0", 0), ("0e22", 0), ("0e23", INEXACT), ("-0", NEGZERO), ("-0.0", NEGZERO), ("-.0", NEGZERO), ("-0e0", NEGZERO),
    ("-0.000", NEGZERO), ("-5", 0), ("+5", TOKEN), ("+5.5", TOKEN), ("5e+2", 0), ("5E-2", 0), ("5e", TOKEN), ("5e+", TOKEN),
    ("e5", TOKEN), (".", TOKEN), ("-", TOKEN), ("5..5", TOKEN), ("1e0001", 0), ("1e00001", TOKEN), ("5e5e5", TOKEN), ("--5", TOKEN),
])
def test_the_real_window_edges(token, kind):
    got, val = _values([token], 1)
    assert got[0] == kind
    if kind == 0:
        assert val[0] == _mmread_row([token], np.array([True]), 1).view(np.int64)[0]


@pytest.mark.parametrize("token,kind", [
    ("0", 0), ("-0", 0), ("007", 0), ("999999999999999999", 0), ("-999999999999999999", 0), ("1000000000000000000", TOKEN),
    ("+5", TOKEN), ("5.", TOKEN), ("5.5", TOKEN), ("5e1", TOKEN), ("-", TOKEN), ("--5", TOKEN), ("5-", TOKEN),
])
def test_the_integer_token_edges(token, kind):
    got, val = _values([token], 0)
    assert got[0] == kind
    if kind == 0:
        assert val[0] == _mmread_row([token], np.array([True]), 0)[0]


B = b"%%MatrixMarket matrix coordinate integer general\n"


@pytest.mark.parametrize("head,want", [
    (B + b"3 4 2\n", (0, 3, 4, 2, 1)),
    (B.replace(b"integer", b"real") + b"%c\n%\n3 4 2\n", (1, 3, 4, 2, 3)),
    (b"%%MatrixMarket MATRIX Coordinate Real GENERAL\n3 4 2\n", (1, 3, 4, 2, 1)),
    (b"%%MatrixMarket  matrix\tcoordinate integer general \r\n% c\r\n 3\t4  2 \r\n", (0, 3, 4, 2, 2)),
    (B + b"%" + b"x" * 5000 + b"\n3 4 0", (0, 3, 4, 0, 2)),
    (B + b"003 04 000000000000000002\n", (0, 3, 4, 2, 1)),
    (b"%%matrixmarket matrix coordinate integer general\n3 4 2\n", 1),      # (scipy wants this word as it is spelt)
    (b" " + B + b"3 4 2\n", 1),
    (B.replace(b"integer", b"pattern") + b"3 4 2\n", 1),
    (B.replace(b"integer", b"complex") + b"3 4 2\n", 1),
    (B.replace(b"coordinate", b"array") + b"3 4\n", 1),
    (B.replace(b"general", b"symmetric") + b"3 3 2\n", 1),
    (B.replace(b"general", b"skew-symmetric") + b"3 3 2\n", 1),
    (B.replace(b"general", b"hermitian") + b"3 3 2\n", 1),
    (B[:-1], 1),
    (b"", 1),
    (B, 2),
    (B + b"%c\n", 3),
    (B + b"%c", 2),
    (B + b"\n3 4 2\n", 2),
    (B + b"%c\n\n3 4 2\n", 3),
    (B + b"0 4 0\n", 2),
    (B + b"3 0 0\n", 2),
    (B + b"3 4\n", 2),
    (B + b"3 4 2 1\n", 2),
    (B + b"3 4 -2\n", 2),
    (B + b"3 4 2.0\n", 2),
    (B + b"3 4 1234567890123456789\n", 2),
    (B + b" %c\n3 4 2\n", 2),
    (B + b"3 4 2\r", 2),
])
def test_header_forms(head, want):
    from cytospace_amd.common import parse_mtx_header
    got = parse_mtx_header(head + (b"1 1 1\n" if head.endswith(b"\n") and not isinstance(want, int) else b""),
                           len(head) + (6 if head.endswith(b"\n") and not isinstance(want, int) else 0))
    if isinstance(want, int):
        assert got == want
    else:
        assert (got["field"], got["G"], got["C"], got["nnz"], got["lines"] - 1) == want
        assert got["data_offset"] == len(head)


def test_header_must_end_within_the_first_mib():
    from cytospace_amd.common import parse_mtx_header
    head = B + b"%" + b"x" * (1 << 20) + b"\n3 4 0\n"
    assert parse_mtx_header(head[:1 << 20], len(head)) == 2


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_model_against_read_file(tmp_path, case):
    from cytospace_amd.common import _mtx_frame, _mtx_labels, parse_mtx_header, read_file
    path = mm.write_case(str(tmp_path), case)
    h = parse_mtx_header(case.data, len(case.data))
    assert (h["field"], h["G"], h["C"], h["nnz"], h["data_offset"]) == (case.field, case.G, case.C, case.nnz, case.d0)
    m = mm.mtx_model(case.data, case.d0, case.G, case.C, case.nnz, case.field)
    if case.intended != "device":
        assert m["status"] == 7 and m["reason"] == case.intended
        return
    assert m["status"] == 0, m.get("reason")
    genes, cells, _, _ = _mtx_labels(path)
    _equal(_mtx_frame(genes, cells, m["words"], case.field), read_file(path, keep_sparse=False))


def test_every_refusal_kind_is_planted():
    kinds = {c.intended[0] for c in CASES if c.intended != "device"}
    assert kinds == set(mm.KIND_NAMES.values()) - {"io", "memory"}


def _dir(tmp_path, text, genes=2, cells=3, name="matrix.mtx"):
    (tmp_path / "genes.tsv").write_text("".join(f"g{i}\n" for i in range(genes)))
    (tmp_path / "barcodes.tsv").write_text("".join(f"c{i}\n" for i in range(cells)))
    p = tmp_path / name
    p.write_bytes(text)
    return str(p)


def _host(path, kind):
    """A file that never reaches the device: read_mtx_device gives read_file's frame or its exception, and says why."""
    from cytospace_amd.common import read_file, read_mtx_device
    try:
        want = read_file(path, keep_sparse=False)
    except Exception as e:
        with pytest.raises(type(e)) as got:
            read_mtx_device(path)
        assert str(got.value) == str(e)
        return
    got, info = read_mtx_device(path, return_info=True)
    assert info["path"] == "scipy" and info["reason"]["kind"] == kind and info["total_s"] > 0
    _equal(got, want)


def test_files_outside_the_header_grammar_are_read_by_read_file(tmp_path):
    body = b"2 3 2\n1 1 5\n2 3 7\n"
    for k, (text, kind) in enumerate([
            (B.replace(b"integer", b"pattern") + b"2 3 2\n1 1\n2 3\n", "header"),
            (B.replace(b"general", b"symmetric").replace(b"2 3", b"3 3") + b"3 3 1\n2 1 5\n", "header"),
            (b"%%MatrixMarket matrix array integer general\n2 3\n1\n2\n3\n4\n5\n6\n", "header"),
            (B + b"\n" + body, "header"),
            (B + b"2 4 1\n1 1 5\n", "shape"),
            (B + b"3 3 1\n1 1 5\n", "shape"),
            (b"%%matrixmarket matrix coordinate integer general\n" + body, "header"),
            (b"not a matrix\n", "header")]):
        d = tmp_path / f"d{k}"
        d.mkdir()
        _host(_dir(d, text, genes=3 if b"symmetric" in text else 2), kind)


def test_compressed_missing_and_unlabelled_files_are_read_by_read_file(tmp_path):
    text = B + b"2 3 2\n1 1 5\n2 3 7\n"
    gz = tmp_path / "gz"
    gz.mkdir()
    _host(_dir(gz, gzip.compress(text), name="matrix.mtx.gz"), "compressed")
    _host(str(tmp_path / "nowhere" / "matrix.mtx"), "io")
    bare = tmp_path / "bare"
    bare.mkdir()
    (bare / "matrix.mtx").write_bytes(text)
    _host(str(bare / "matrix.mtx"), "labels")
    half = tmp_path / "half"
    half.mkdir()
    (half / "matrix.mtx").write_bytes(text)
    (half / "features.csv").write_text("g0\ng1\n")
    _host(str(half / "matrix.mtx"), "labels")
    dup = tmp_path / "dup"
    dup.mkdir()
    p = _dir(dup, text)
    (dup / "barcodes.tsv").write_text("c0\nc1\nc0\n")           # (read_file's own frame for repeated cell labels, whatever it is)
    _host(p, "labels")
    _host(str(tmp_path / "table.tsv"), "not matrix market")


def test_bad_arguments_are_refused_before_any_device_is_touched(tmp_path):
    from cytospace_amd import _lib
    L = _lib.lib()
    path = _dir(tmp_path, B + b"2 3 1\n1 1 5\n").encode()
    out = np.zeros((2, 3), np.int64)
    info = _lib.MtxReadInfo()
    good = dict(path=path, off=len(B) + 6, G=2, C=3, nnz=1, field=0, out=out.ctypes.data, ldo=3, info=ctypes.byref(info))
    for change in (dict(path=None), dict(out=None), dict(info=None), dict(G=0), dict(G=-1), dict(C=0), dict(nnz=-1), dict(off=-1),
                   dict(ldo=2), dict(field=2), dict(field=-1)):
        a = {**good, **change}
        st = L.cyto_mtx_read(a["path"], a["off"], a["G"], a["C"], a["nnz"], a["field"], a["out"], a["ldo"], 0, a["info"])
        assert st == 1, change                                                   # CYTO_ERR_BAD_ARG
    assert not out.any()
    z = np.zeros(1, np.int64)
    k = np.zeros(1, np.int8)
    text = ctypes.create_string_buffer(b"1 1 5")
    off = np.array([0, 5], np.int64)
    ok = [text, 1, off.ctypes.data, 0, 1, 1, k.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data]
    assert L.cyto_mtx_parse_entries(*ok) == 0
    for pos, bad in ((1, -1), (3, 2), (0, None), (6, None), (10, None)):
        a = list(ok)
        a[pos] = bad
        assert L.cyto_mtx_parse_entries(*a) == 1
    assert L.cyto_mtx_parse_entries(None, 0, None, 0, 1, 1, None, None, None, None, None) == 0
