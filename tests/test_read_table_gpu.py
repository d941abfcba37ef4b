"""read_file_device (C ABI: cyto_table_read / cyto_table_fetch; csrc/table.hip) against read_file on the GPU: tables in the
device grammar come back equal through the device path (index, columns, dtypes, values bit for bit); files outside it are read
by read_file itself, with its result or its exception."""
import gzip
import os

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu


def _equal(a, b):
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    for c in range(a.shape[1]):
        x, y = a.iloc[:, c].to_numpy(), b.iloc[:, c].to_numpy()
        assert x.dtype == y.dtype
        if x.dtype == np.float64:
            assert np.array_equal(x.view(np.int64), y.view(np.int64))


def _device(path):
    from cytospace_amd.common import read_file, read_file_device
    got, info = read_file_device(str(path), return_info=True)
    assert info["path"] == "device", info.get("reason")
    _equal(got, read_file(str(path)))
    for k in ("file_read_s", "upload_s", "kernels_s", "download_s", "dataframe_s"):
        assert info[k] >= 0
    return got


def _fallback(path):
    from cytospace_amd.common import read_file, read_file_device
    try:
        want = read_file(str(path))
    except Exception as e:
        with pytest.raises(type(e)):
            read_file_device(str(path))
        return None
    got, info = read_file_device(str(path), return_info=True)
    assert info["path"] == "pandas"
    _equal(got, want)
    return info["reason"]


def _frame(rng, G, C, kind):
    if kind == "int":
        v = rng.poisson(0.4, (G, C))
    elif kind == "float":
        v = rng.normal(0, 1, (G, C)) * 10.0 ** rng.integers(-8, 8, (G, C))
        v[0, 0] = -0.0
    else:
        v = rng.poisson(3, (G, C)).astype(object)
        v[:, 1::3] = rng.normal(0, 100, (G, len(range(1, C, 3))))
    return pd.DataFrame(v, index=pd.Index([f"g{i}" for i in range(G)], name="ID"), columns=[f"c{j}" for j in range(C)])


@pytest.mark.parametrize("ext", ["tsv", "csv", "txt"])
@pytest.mark.parametrize("kind", ["int", "float", "mixed"])
def test_to_csv_tables(tmp_path, ext, kind):
    rng = np.random.default_rng(len(ext) * 7 + len(kind))
    p = tmp_path / f"t.{ext}"
    _frame(rng, 37, 53, kind).to_csv(p, sep="," if ext == "csv" else "\t")
    got = _device(p)
    assert got.shape == (37, 53)


def test_crlf_and_no_final_newline(tmp_path):
    rng = np.random.default_rng(1)
    p = tmp_path / "crlf.csv"
    _frame(rng, 20, 9, "mixed").to_csv(p, lineterminator="\r\n")
    _device(p)
    q = tmp_path / "open.tsv"
    q.write_bytes(b"ID\ta\tb\nx\t1\t2.5\ny\t3\t4")
    _device(q)
    r = tmp_path / "open_crlf.tsv"
    r.write_bytes(b"ID\ta\tb\r\nx\t1\t2.5\r\ny\t3\t4\r\n")
    _device(r)


def test_r_write_table_header(tmp_path):
    p = tmp_path / "scRNA_data.txt"           # write.table(..., sep='\t', quote=F): one header field fewer than the data lines
    p.write_bytes(b"cellA\tcellB\tcellC\nGAPDH\t5\t0\t12\nACTB\t0\t1\t3\nMT-CO1\t7\t8\t9\n")
    got = _device(p)
    assert got.index.name is None and list(got.columns) == ["cellA", "cellB", "cellC"]


def test_duplicates_and_labels(tmp_path):
    p = tmp_path / "dup.tsv"
    p.write_bytes(b"ID\ta\ta\tb\ta\nx\t1\t2\t3\t4\nx\t5\t6\t7\t8\ny\t9\t10\t11\t12\n")
    got = _device(p)
    assert list(got.columns) == ["a", "a.1", "b", "a.2"] and list(got.index) == ["x", "x", "y"]
    q = tmp_path / "intlab.csv"
    q.write_bytes(b"gene,a,b\n10,1,2\n20,3,4\n10,5,6\n")
    assert _device(q).index.dtype == np.int64
    r = tmp_path / "nalab.csv"
    r.write_bytes(b"gene,a\n1,1\nNA,2\n3,3\n,4\n")
    assert _device(r).index.dtype == np.float64
    s = tmp_path / "odd.tsv"
    s.write_bytes(b"ID\tv\n  spaced\t1\n7SK\t2\ng-1.x\t3\n\xc3\xa9t\xc3\xa9\t4\n")
    _device(s)


def test_tokens_in_the_grammar(tmp_path):
    p = tmp_path / "tok.tsv"
    p.write_bytes(b"ID\ti\tf\tg\th\tz\n"
                  b"a\t+5\t5.\t-0.5\t1e5\t-0\n"
                  b"b\t007\t.5\t-0.0\t1E-5\t-00\n"
                  b"c\t-999999999999999999\t-.25\t0\t2.5e+300\t+0\n"
                  b"d\t999999999999999999\t1\t3\t1e-320\t0\n")
    got = _device(p)
    assert list(got.dtypes) == [np.int64, np.float64, np.float64, np.float64, np.int64]
    assert np.signbit(got["g"].iloc[1]) and not np.signbit(got["g"].iloc[2])


def test_one_row_one_column(tmp_path):
    p = tmp_path / "one.tsv"
    p.write_bytes(b"ID\tonly\nx\t42\n")
    assert _device(p).shape == (1, 1)


def test_wide_table(tmp_path):
    rng = np.random.default_rng(5)
    p = tmp_path / "wide.tsv"
    _frame(rng, 12, 20000, "int").to_csv(p, sep="\t")
    got = _device(p)
    assert got.shape == (12, 20000)


@pytest.mark.parametrize("name,text,kind", [
    ("quoted.csv", b'ID,a\n"x",1\ny,2\n', "quote"),
    ("na.tsv", b"ID\ta\tb\nx\tNA\t1\ny\t2\t3\n", "token"),
    ("empty.csv", b"ID,a,b\nx,,1\ny,2,3\n", "token"),
    ("ragged_short.tsv", b"ID\ta\tb\nx\t1\t2\ny\t3\n", "field count"),
    ("ragged_long.tsv", b"ID\ta\tb\nx\t1\t2\ny\t3\t4\t5\n", "field count"),
    ("blank.tsv", b"ID\ta\nx\t1\n\ny\t2\n", "blank line"),
    ("int19.tsv", b"ID\ta\nx\t1234567890123456789\ny\t1\n", "token"),
    ("big.tsv", b"ID\ta\nx\t1e400\ny\t1\n", "out of range"),
    ("text.tsv", b"ID\ta\nx\tabc\n", "token"),
    ("wideint.tsv", b"ID\ta\nx\t12345678901234567\ny\t0.5\n", "integer cast in a float column"),
    ("negzero.tsv", b"ID\ta\nx\t-0\ny\t0.5\n", "integer cast in a float column"),
    ("castlabel.tsv", b"ID\ta\n12345678901234567\t1\nNA\t2\n", "row labels"),
    ("negzerolabel.tsv", b"ID\ta\n-0\t1\nNA\t2\n", "row labels"),
])
def test_outside_the_grammar_falls_back(tmp_path, name, text, kind):
    p = tmp_path / name
    p.write_bytes(text)
    reason = _fallback(p)
    if reason is not None:
        assert reason["kind"] == kind


def test_gzip_matrix_market_and_no_columns_fall_back(tmp_path):
    import scipy.io
    import scipy.sparse as sp
    p = tmp_path / "t.tsv.gz"
    with gzip.open(p, "wb") as f:
        f.write(b"ID\ta\tb\nx\t1\t2\n")
    assert _fallback(p)["kind"] == "compressed"
    scipy.io.mmwrite(str(tmp_path / "matrix.mtx"), sp.csc_matrix(np.array([[1, 0, 2], [0, 3, 0]])))
    (tmp_path / "genes.tsv").write_text("g1\ng2\n")
    (tmp_path / "barcodes.tsv").write_text("c1\nc2\nc3\n")
    from cytospace_amd.common import read_file, read_file_device
    got, info = read_file_device(str(tmp_path / "matrix.mtx"), return_info=True)
    assert info["path"] == "pandas" and info["reason"]["kind"] == "matrix market"
    _equal(got, read_file(str(tmp_path / "matrix.mtx"), keep_sparse=False))
    q = tmp_path / "nocols.tsv"
    q.write_bytes(b"ID\nx\ny\n")
    assert _fallback(q)["kind"] == "no data columns"


def _wide_with(tmp_path, name, tokens, rows=40, cols=20000):
    """A table wide enough that pandas converts it in blocks of a few rows; column 0 holds `tokens` (row -> token), "1" elsewhere."""
    body = [["1"] * cols for _ in range(rows)]
    for r, tok in tokens.items():
        body[r][0] = tok
    p = tmp_path / name
    p.write_text("ID\t" + "\t".join(f"c{j}" for j in range(cols)) + "\n" +
                 "".join(f"g{r}\t" + "\t".join(body[r]) + "\n" for r in range(rows)))
    return p


def test_integer_tokens_of_a_float_column_across_pandas_blocks(tmp_path):
    # pandas reads a block of rows without a decimal token in c0 as int64 and casts it to float64: "-0" becomes +0.0 there and a
    # 17-digit integer is rounded by the cast, not by the decimal converter.  Such columns are read by pandas.
    for name, tok in (("negzero.tsv", "-0"), ("digits17.tsv", "12345678901234567")):
        p = _wide_with(tmp_path, name, {0: tok, 39: "0.25"})
        assert _fallback(p)["kind"] == "integer cast in a float column"
    # the same tokens in a column of integers only, and "-0.0" beside a decimal token, stay on the device
    _device(_wide_with(tmp_path, "ints.tsv", {0: "-0", 5: "12345678901234567"}))
    got = _device(_wide_with(tmp_path, "negzero_dec.tsv", {0: "-0.0", 39: "0.25"}))
    assert np.signbit(got["c0"].iloc[0])


def test_file_of_several_upload_chunks(tmp_path):
    # 40 MB: three 16 MiB chunks, so the double-buffered upload waits for and reuses its pinned buffers
    rng = np.random.default_rng(9)
    G, C = 2000, 10000
    p = tmp_path / "big.tsv"
    row = np.empty(2 * C + 1, np.uint8)
    row[0:2 * C:2] = ord("\t")
    row[2 * C] = ord("\n")
    with open(p, "wb") as f:
        f.write(("\t".join(f"cell{j}" for j in range(C)) + "\n").encode())
        for g in range(G):
            row[1:2 * C:2] = ord("0") + rng.integers(0, 10, C)
            f.write(f"gene{g}".encode() + row.tobytes())
    assert os.path.getsize(p) > 2 * 16 * 2**20
    got = _device(p)
    assert got.shape == (G, C)


def test_read_data_parses_the_expression_tables_on_the_device(tmp_path, monkeypatch):
    from cytospace_amd import common
    from cytospace_amd.cytospace import read_data
    paths = []
    real = common.read_file_device

    def spy(path, device_id=0, return_info=False):
        df, info = real(path, device_id, return_info=True)
        paths.append((path, info["path"]))
        return (df, info) if return_info else df
    monkeypatch.setattr(common, "read_file_device", spy)
    rng = np.random.default_rng(3)
    sc = pd.DataFrame(rng.poisson(2, (30, 8)), index=[f"G{i}" for i in range(30)], columns=[f"c{i}" for i in range(8)])
    st = pd.DataFrame(rng.poisson(5, (30, 4)), index=[f"G{i}" for i in range(30)], columns=[f"s{i}" for i in range(4)])
    sc.to_csv(tmp_path / "sc.tsv", sep="\t")
    st.to_csv(tmp_path / "st.csv")
    pd.DataFrame({"CellType": ["A", "B"] * 4}, index=sc.columns).to_csv(tmp_path / "ct.csv")
    pd.DataFrame({"row": range(4), "col": range(4)}, index=st.columns).to_csv(tmp_path / "xy.csv")
    pd.DataFrame([[0.5, 0.5]], index=["Fraction"], columns=["A", "B"]).to_csv(tmp_path / "fr.csv")
    out = read_data(str(tmp_path / "sc.tsv"), str(tmp_path / "ct.csv"), str(tmp_path / "fr.csv"), None, None, str(tmp_path), "",
                    st_path=str(tmp_path / "st.csv"), coordinates_path=str(tmp_path / "xy.csv"), device_id=0)
    assert sorted(paths) == sorted([(str(tmp_path / "st.csv"), "device"), (str(tmp_path / "sc.tsv"), "device")])
    assert np.array_equal(out[0].to_numpy(), sc.to_numpy()) and np.array_equal(out[2].to_numpy(), st.to_numpy())
