"""read_mtx_device (C ABI: cyto_mtx_read; csrc/mtx_read.hip) against read_file(path, keep_sparse=False) on the GPU: a 10x
directory inside the device grammar comes back equal through the device path (index, columns, dtypes, values bit for bit,
duplicate entries of an integer file summed); a file outside it is read by read_file itself -- its result or its exception --
and the reason names the refusal at the lowest byte.  The generated files and their intended outcomes are those of
tools/mtx_read_model.py, which tests/test_read_mtx_cpu.py holds to read_file without a GPU."""
import json
import os
import threading

import numpy as np
import pandas as pd
import pytest
import scipy.io
import scipy.sparse as sp

from tools import mtx_read_model as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mm.cases()
# (scipy 1.15 reads beyond the end of a file whose last byte is a blank: read_file is not run on those)
SCIPY_SAFE = [c for c in CASES if not c.name.startswith("open_blank")]


def _equal(a, b):
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    x, y = a.to_numpy(), b.to_numpy()
    assert x.dtype == y.dtype and x.dtype in (np.int64, np.float64)
    assert np.array_equal(x.view(np.int64), y.view(np.int64))
    assert list(a.dtypes) == list(b.dtypes)


def _device(path):
    from cytospace_amd.common import read_file, read_mtx_device
    got, info = read_mtx_device(str(path), return_info=True)
    assert info["path"] == "device", info.get("reason")
    _equal(got, read_file(str(path), keep_sparse=False))
    for k in ("labels_s", "header_s", "file_read_s", "upload_s", "kernels_s", "download_s", "dataframe_s", "total_s"):
        assert info[k] >= 0
    return got, info


def _fallback(path):
    """The reason of a file that the device refuses; read_file's own frame or exception comes back."""
    from cytospace_amd.common import _mtx_on_device, read_file, read_mtx_device
    try:
        want = read_file(str(path), keep_sparse=False)
    except Exception as e:
        with pytest.raises(type(e)) as got:
            read_mtx_device(str(path))
        assert str(got.value) == str(e)
        want = None
    info = {}
    assert _mtx_on_device(str(path), 0, info) is None
    if want is not None:
        got, full = read_mtx_device(str(path), return_info=True)
        assert full["path"] == "scipy" and full["reason"] == info["reason"]
        _equal(got, want)
    r = info["reason"]
    return r["kind"], r["line"], r["byte"]


def _tenx(d, matrix_text, G, C):
    d.mkdir(parents=True, exist_ok=True)
    for name, text in mm.label_files(G, C).items():
        (d / name).write_bytes(text)
    (d / "matrix.mtx").write_bytes(matrix_text)
    return d / "matrix.mtx"


def _mmwrite(d, dense):
    d.mkdir(parents=True, exist_ok=True)
    scipy.io.mmwrite(str(d / "matrix.mtx"), sp.coo_matrix(dense))
    for name, text in mm.label_files(*dense.shape).items():
        (d / name).write_bytes(text)
    return d / "matrix.mtx"


@pytest.mark.parametrize("field", ["integer", "real"])
def test_files_written_by_mmwrite(tmp_path, field):
    rng = np.random.default_rng(1)
    dense = rng.poisson(0.5, (37, 53))
    if field == "real":
        dense = np.round(dense * rng.uniform(0.01, 1000.0, dense.shape), 3)
    got, info = _device(_mmwrite(tmp_path, dense))
    assert info["field"] == field and info["entries"] == np.count_nonzero(dense) and info["duplicates"] == 0
    assert np.array_equal(got.to_numpy(), dense) and list(got.index[:2]) == ["g0", "g1"] and list(got.columns[:2]) == ["c0", "c1"]


@pytest.mark.parametrize("field", [0, 1])
def test_small_and_edge_shapes(tmp_path, field):
    v = b"7" if field == 0 else b"7.25"
    for k, (G, C, lines) in enumerate([
            (3, 4, []), (3, 4, [b"3 4 " + v]), (1, 6, [b"1 2 " + v, b"1 6 " + v]), (5, 1, [b"5 1 " + v, b"1 1 " + v]),
            (4, 4, [b"2 2 " + v, b"4 4 " + v]), (1, 1, [b"1 1 " + v]),
            (6, 9, [b"1 1 " + v, b"1 9 " + v, b"6 1 " + v, b"6 9 " + v])]):
        text = mm.header(field, G, C, len(lines)) + b"".join(x + b"\n" for x in lines)
        got, info = _device(_tenx(tmp_path / f"s{k}", text, G, C))
        assert got.shape == (G, C) and info["entries"] == len(lines)
        assert np.count_nonzero(got.to_numpy()) == len(lines)


@pytest.mark.parametrize("variant", ["plain", "long_comment", "no_final_newline", "crlf", "blanks"])
@pytest.mark.parametrize("field", [0, 1])
def test_lines_across_the_blocks_and_thread_spans_of_the_line_pass(tmp_path, field, variant):
    # 12 000 entries of 300 x 400 (about 130 KB): index widths of 1-3 digits put line ends at every residue of the 64 KiB blocks
    # and 256-byte thread spans
    rng = np.random.default_rng(7 + field)
    G, C, nnz = 300, 400, 12000
    lines, _ = mm._entries(rng, field, G, C, nnz, "blanks" if variant == "blanks" else "plain")
    if field == 1:
        lines = mm._real_window_ok(lines)
    eol = b"\r\n" if variant == "crlf" else b"\n"
    comment = b"%" + b"c" * 4998 + eol if variant == "long_comment" else b""
    if variant == "no_final_newline":
        lines[-1] = lines[-1].rstrip(b" \t")
    head = mm.header(field, G, C, nnz, comment, eol)
    text = head + eol.join(lines) + (b"" if variant == "no_final_newline" else eol)
    assert len(text) > 2 * 65536 - 20000 and (variant != "long_comment" or len(head) % 16)
    got, info = _device(_tenx(tmp_path, text, G, C))
    assert info["entries"] == nnz


def test_file_of_several_upload_chunks(tmp_path):
    # more than 32 MiB of text: three 16 MiB chunks, so the double-buffered upload waits for and reuses its pinned buffers
    rng = np.random.default_rng(9)
    G, C = 2000, 10000
    r, c = np.nonzero(rng.random((G, C)) < 0.16)
    order = rng.permutation(len(r))
    v = rng.integers(1, 1000, len(r))
    path = _tenx(tmp_path, mm.header(0, G, C, len(r)), G, C)
    pd.DataFrame({"r": r[order] + 1, "c": c[order] + 1, "v": v}).to_csv(path, sep=" ", header=False, index=False, mode="a")
    assert os.path.getsize(path) > 2 * 16 * 2**20 and len(r) > 3_000_000
    got, info = _device(path)
    assert info["entries"] == len(r) and np.array_equal(got.to_numpy()[r, c], v[np.argsort(order)])


def test_duplicate_entries(tmp_path):
    rng = np.random.default_rng(3)
    G, C = 40, 50
    lines = [x.rsplit(b" ", 1)[0] + b" %d" % (k % 9 + 1) for k, x in enumerate(mm._entries(rng, 0, G, C, 600, "plain")[0])]
    first = lines[0].rsplit(b" ", 1)[0]
    lines[5] = lines[4].rsplit(b" ", 1)[0] + b" 11"                                  # a pair
    lines[100] = lines[101] = lines[300].rsplit(b" ", 1)[0] + b" 13"                 # a triple with line 300
    lines[-1] = first + b" 17"                                                       # the first and the last line
    text = mm.header(0, G, C, len(lines)) + b"".join(x + b"\n" for x in lines)
    got, info = _device(_tenx(tmp_path / "int", text, G, C))
    m = mm.mtx_model(text, len(mm.header(0, G, C, len(lines))), G, C, len(lines), 0)
    assert np.array_equal(got.to_numpy(), m["words"])
    assert info["duplicates"] == m["duplicates"] == 4         # (every value is positive: entries minus distinct cells)
    real = [x.rsplit(b" ", 1)[0] + b" 2.5" for x in lines]
    head = mm.header(1, G, C, len(real))
    text = head + b"".join(x + b"\n" for x in real)
    kind, line, byte = _fallback(_tenx(tmp_path / "real", text, G, C))
    assert (kind, line) == ("duplicate entry", 3 + 5 + 1) and byte == len(head) + sum(len(x) + 1 for x in real[:5])


@pytest.mark.parametrize("case", SCIPY_SAFE, ids=[c.name for c in SCIPY_SAFE])
def test_generated_files(tmp_path, case):
    path = mm.write_case(str(tmp_path), case)
    if case.intended == "device":
        got, info = _device(path)
        m = mm.mtx_model(case.data, case.d0, case.G, case.C, case.nnz, case.field)
        assert np.array_equal(got.to_numpy().view(np.int64), m["words"]) and info["entries"] == case.nnz
    else:
        assert _fallback(path) == case.intended


def test_a_blank_that_ends_the_file_is_refused(tmp_path):
    from cytospace_amd.common import _mtx_on_device
    for case in (c for c in CASES if c.name.startswith("open_blank")):
        info = {}
        assert _mtx_on_device(mm.write_case(str(tmp_path / case.name), case), 0, info) is None
        r = info["reason"]
        assert (r["kind"], r["line"], r["byte"]) == case.intended


def test_every_refusal_kind_has_a_file():
    assert {c.intended[0] for c in CASES if c.intended != "device"} == set(mm.KIND_NAMES.values()) - {"io", "memory"}


def test_poisoned_work_buffers(tmp_path):
    from cytospace_amd import _lib
    from cytospace_amd.common import read_mtx_device
    rng = np.random.default_rng(5)
    paths = [_mmwrite(tmp_path / "i", rng.poisson(0.3, (70, 90))), _mmwrite(tmp_path / "r", rng.poisson(0.3, (70, 90)) * 0.5)]
    clean = [read_mtx_device(str(p)) for p in paths]
    _lib.cache_poison(0xA5)
    try:
        for p, want in zip(paths, clean):
            got, info = read_mtx_device(str(p), return_info=True)
            assert info["path"] == "device"
            _equal(got, want)
    finally:
        _lib.cache_poison(None)


def test_repeated_and_concurrent_calls(tmp_path):
    from cytospace_amd.common import read_mtx_device
    rng = np.random.default_rng(6)
    path = str(_mmwrite(tmp_path, rng.poisson(0.2, (400, 700))))
    first, _ = _device(path)
    for _ in range(5):
        _equal(read_mtx_device(path), first)
    out = [None, None]

    def run(k):
        out[k] = read_mtx_device(path, return_info=True)
    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for got, info in out:
        assert info["path"] == "device"
        _equal(got, first)


def _stage_gv14(d):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "gv14_main.npz"))
    tag = "visium_ncpsp"
    for k in gold.files:
        if k.startswith(f"{tag}::in::"):
            (d / k.split("::")[2]).write_bytes(gold[k].tobytes())
    args = json.loads(gold[f"{tag}::args"].tobytes().decode())
    args["solver_method"] = "lapjv_hip"
    return args


def _as_tenx(table_path, d):
    """The counts of a delimited scRNA table as a 10x directory; returns the path of matrix.mtx."""
    from cytospace_amd.common import read_file
    df = read_file(str(table_path), keep_sparse=False)
    d.mkdir()
    scipy.io.mmwrite(str(d / "matrix.mtx"), sp.coo_matrix(df.to_numpy()))
    (d / "features.tsv").write_text("".join(f"{g}\n" for g in df.index))
    (d / "barcodes.tsv").write_text("".join(f"{c}\n" for c in df.columns))
    return d / "matrix.mtx"


def test_read_data_reads_a_10x_directory_on_the_device(tmp_path, monkeypatch):
    from cytospace_amd import common
    from cytospace_amd.cytospace import read_data
    calls = []
    real = common.read_mtx_device

    def spy(path, device_id=0, return_info=False):
        df, info = real(path, device_id, return_info=True)
        calls.append((path, info["path"]))
        return (df, info) if return_info else df
    monkeypatch.setattr(common, "read_mtx_device", spy)
    rng = np.random.default_rng(3)
    sc = pd.DataFrame(rng.poisson(2, (30, 8)), index=[f"G{i}" for i in range(30)], columns=[f"c{i}" for i in range(8)])
    st = pd.DataFrame(rng.poisson(5, (30, 4)), index=[f"G{i}" for i in range(30)], columns=[f"s{i}" for i in range(4)])
    sc.to_csv(tmp_path / "sc.tsv", sep="\t")
    mtx = _as_tenx(tmp_path / "sc.tsv", tmp_path / "tenx")
    st.to_csv(tmp_path / "st.csv")
    pd.DataFrame({"CellType": ["A", "B"] * 4}, index=sc.columns).to_csv(tmp_path / "ct.csv")
    pd.DataFrame({"row": range(4), "col": range(4)}, index=st.columns).to_csv(tmp_path / "xy.csv")
    pd.DataFrame([[0.5, 0.5]], index=["Fraction"], columns=["A", "B"]).to_csv(tmp_path / "fr.csv")
    out = read_data(str(mtx), str(tmp_path / "ct.csv"), str(tmp_path / "fr.csv"), None, None, str(tmp_path), "",
                    st_path=str(tmp_path / "st.csv"), coordinates_path=str(tmp_path / "xy.csv"), device_id=0)
    assert calls == [(str(mtx), "device")]
    assert np.array_equal(out[0].to_numpy(), sc.to_numpy()) and list(out[0].columns) == ["CELL_" + c for c in sc.columns]


def test_main_cytospace_from_a_10x_directory_writes_the_same_files(tmp_path, monkeypatch):
    from cytospace_amd import common
    from cytospace_amd.cytospace import main_cytospace
    args = _stage_gv14(tmp_path)
    mtx = _as_tenx(tmp_path / args["scRNA_path"], tmp_path / "tenx")
    paths = []
    real = common.read_mtx_device

    def spy(path, device_id=0, return_info=False):
        df, info = real(path, device_id, return_info=True)
        paths.append(info["path"])
        return (df, info) if return_info else df
    monkeypatch.setattr(common, "read_mtx_device", spy)
    monkeypatch.chdir(tmp_path)
    files = {}
    for tag, sc in (("table", args["scRNA_path"]), ("tenx", os.path.relpath(mtx, tmp_path))):
        main_cytospace(**dict(args, scRNA_path=sc, output_folder="out_" + tag))
        d = tmp_path / ("out_" + tag)
        files[tag] = {os.path.relpath(os.path.join(r, f), d): open(os.path.join(r, f), "rb").read()
                      for r, _, fs in os.walk(d) for f in fs}
    assert paths == ["device"]
    assert sorted(files["table"]) == sorted(files["tenx"]) and "assigned_locations.csv" in files["tenx"]
    for name, data in files["table"].items():
        if name != "log.txt":                                   # (the log names the input path, the folder and the run time)
            assert files["tenx"][name] == data, name
