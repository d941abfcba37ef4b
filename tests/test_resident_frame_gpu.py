"""resident.DeviceFrame through the stages that take one, each against the same stage's DataFrame call: the reader
(read_file_device(resident=True).to_frame() is read_file_device's frame), downsampling (the frame, the words and numpy's global
state), apply_linear_assignment in its three forms, and the MatrixMarket writer (the same bytes).  Nothing has a tolerance."""
import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

from cytospace_amd import resident
from cytospace_amd.common import downsample_device, read_file_device
from cytospace_amd.cytospace import apply_linear_assignment
from cytospace_amd.post_processing import write_mtx_device


def _table(path, values, sep=",", fmt=str):
    G, C = values.shape
    with open(path, "w") as f:
        f.write(sep.join(["gene"] + [f"c{j}" for j in range(C)]) + "\n")
        for g in range(G):
            f.write(sep.join([f"g{g}"] + [fmt(v) for v in values[g]]) + "\n")
    return str(path)


def _counts(G=37, C=53, seed=0):
    return np.random.default_rng(seed).poisson(2.0, (G, C)).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["csv of ints", "csv of decimals", "tsv"])
def test_reader_keeps_the_table_on_the_device(kind, tmp_path, hip_lib):
    x = _counts()
    if kind == "csv of decimals":
        p = _table(tmp_path / "t.csv", x / 8.0, fmt=lambda v: repr(float(v)))
    elif kind == "tsv":
        p = _table(tmp_path / "t.tsv", x, sep="\t")
    else:
        p = _table(tmp_path / "t.csv", x)
    want, winfo = read_file_device(p, return_info=True)
    frame, info = read_file_device(p, return_info=True, resident=True)
    assert winfo["path"] == "device" and winfo["resident"] is False and isinstance(want, pd.DataFrame)
    assert isinstance(frame, resident.DeviceFrame) and info["resident"] is True and info["path"] == "device"
    assert frame.source == "table" and frame.fetches == 0 and frame.shape == want.shape
    assert frame.dtype == (np.float64 if kind == "csv of decimals" else np.int64)
    assert frame.index.equals(want.index) and frame.columns.equals(want.columns) and frame.index.name == want.index.name
    assert_frame_equal(frame.to_frame(), want, check_exact=True)
    assert frame.fetches == 1
    # a view: rows and columns out of order, with repeats
    rows, cols = np.array([5, 0, 36, 5]), np.array([52, 1, 1, 0, 17])
    view = frame.take(rows, cols)
    assert_frame_equal(view.to_frame(), want.iloc[rows, cols], check_exact=True)
    assert frame.fetches == 2 and view.stats is frame.stats
    r = view.value_range()
    v = want.iloc[rows, cols].to_numpy()
    assert (r["lo"], r["hi"]) == (v.min(), v.max())
    frame.close()
    with pytest.raises(RuntimeError):
        frame.to_frame()


@pytest.mark.gpu
def test_tables_a_frame_cannot_stand_for_come_back_as_dataframes(tmp_path, hip_lib):
    x = _counts(9, 4).astype(object)
    x[:, 2] = [v + 0.5 for v in x[:, 2]]
    mixed = _table(tmp_path / "mixed.csv", x)
    df, info = read_file_device(mixed, return_info=True, resident=True)
    assert isinstance(df, pd.DataFrame) and info["path"] == "device" and info["resident"] is False
    assert info["resident_reason"] == "mixed column kinds"
    assert_frame_equal(df, read_file_device(mixed), check_exact=True)
    assert sorted(str(t) for t in df.dtypes.unique()) == ["float64", "int64"]
    quoted = tmp_path / "quoted.csv"
    quoted.write_text('gene,a,b\n"g0",1,2\ng1,3,4\n')
    df, info = read_file_device(str(quoted), return_info=True, resident=True)
    assert isinstance(df, pd.DataFrame) and info["path"] == "pandas" and info["resident"] is False
    assert_frame_equal(df, pd.read_csv(quoted, index_col=0), check_exact=True)
    dup = tmp_path / "dup.csv"
    dup.write_text("gene,a,a\ng0,1,2\ng1,3,4\n")
    # (pandas' header parse mangles a repeated name, so the reader's labels are unique and a frame stands for the table; a
    #  DataFrame that does carry a label twice is not taken)
    frame = read_file_device(str(dup), resident=True)
    assert isinstance(frame, resident.DeviceFrame) and list(frame.columns) == ["a", "a.1"]
    assert_frame_equal(frame.to_frame(), read_file_device(str(dup)), check_exact=True)
    with pytest.raises(TypeError, match="duplicate column labels"):
        resident.DeviceFrame.from_frame(pd.DataFrame([[1, 2]], columns=["a", "a"]))
    with pytest.raises(TypeError, match="dtypes"):
        resident.DeviceFrame.from_frame(pd.DataFrame({"a": [1], "b": [0.5]}))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int64, np.uint16])
def test_downsample_of_a_view_equals_the_dataframe_call(dtype, hip_lib):
    G, C = 41, 67
    x = np.random.default_rng(1).poisson(6.0, (G, C)).astype(np.int64)
    df = pd.DataFrame(x, index=[f"g{i}" for i in range(G)], columns=[f"c{j}" for j in range(C)])
    perm = np.random.default_rng(2).permutation(C)
    rows = np.r_[np.arange(3, G), 0]
    frame = resident.DeviceFrame.from_frame(df).take(rows, perm)
    host = df.iloc[rows, perm]
    assert frame.source == "upload"
    np.random.seed(77)
    np.random.normal()                                         # (has_gauss and the cached value must survive)
    start = np.random.get_state()
    want, want_words = downsample_device(host, 150, dtype=dtype, return_words=True)
    want_state = np.random.get_state()
    np.random.set_state(start)
    got, got_words = downsample_device(frame, 150, dtype=dtype, return_words=True)
    got_state = np.random.get_state()
    assert isinstance(got, resident.DeviceFrame) and got.dtype == np.dtype(dtype) and got.fetches == 0
    assert want_words > 0 and got_words == want_words
    assert got_state[0] == want_state[0] and np.array_equal(got_state[1], want_state[1]) and got_state[2:] == want_state[2:]
    assert_frame_equal(got.to_frame(), want, check_exact=True)
    assert got.stats is frame.stats and frame.materialized == 1
    with pytest.raises(ValueError):
        downsample_device(frame, -1)
    with pytest.raises(ValueError):
        downsample_device(frame, 70000, dtype=np.uint16)
    fl = resident.DeviceFrame.from_frame(df.astype(np.float64))
    with pytest.raises(TypeError):
        downsample_device(fl, 10)
    neg = x.copy()
    neg[0, 0] = -1
    state = np.random.get_state()
    with pytest.raises(ValueError, match="negative count"):
        downsample_device(resident.DeviceFrame.from_frame(pd.DataFrame(neg)), 10)
    now = np.random.get_state()
    assert np.array_equal(now[1], state[1]) and now[2:] == state[2:]


@pytest.fixture(scope="module")
def assignment_inputs():
    G, C, S = 60, 120, 40
    rng = np.random.default_rng(8)
    profiles = rng.gamma(0.7, 3.0, (G, 6))
    sc = rng.poisson(profiles[:, rng.integers(0, 6, C)]).astype(np.int64)
    st = rng.poisson(3.0 * profiles[:, rng.integers(0, 6, S)]).astype(np.int64)
    sc_df = pd.DataFrame(sc, index=[f"g{i}" for i in range(G)], columns=[f"CELL_{j}" for j in range(C)])
    st_df = pd.DataFrame(st, index=sc_df.index, columns=[f"SPOT_{j}" for j in range(S)])
    coords = pd.DataFrame({"row": np.arange(S) // 8, "col": np.arange(S) % 8}, index=st_df.columns)
    return sc_df, st_df, coords, np.full(S, 3, np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "index_st_list", "sub_spots"])
def test_apply_linear_assignment_takes_frames(form, assignment_inputs, hip_lib):
    sc_df, st_df, coords, slots = assignment_inputs
    C, S = sc_df.shape[1], st_df.shape[1]
    kw = {}
    if form == "plain":
        index_sc = [np.arange(C)]
    elif form == "index_st_list":
        st_df, coords, slots = st_df, coords, np.ones(S, np.int64)
        sc_df = sc_df.iloc[:, :S]
        order = np.random.default_rng(4).permutation(S)
        index_sc = [np.arange(0, 17), np.arange(17, S)]
        kw["index_st_list"] = [order[:17], order[17:]]
    else:
        index_sc = [np.arange(0, 60), np.arange(60, C)]
        spot_of_slot = np.random.default_rng(5).permutation(np.repeat(np.arange(S), slots))
        kw["subsampled_cell_number_to_node_assignment_list"] = [np.bincount(spot_of_slot[:60], minlength=S),
                                                                np.bincount(spot_of_slot[60:], minlength=S)]
    args = (coords, slots, "lapjv_hip", None, 1, "Pearson_correlation", 2, index_sc)
    want_loc, want_ids = apply_linear_assignment(sc_df, st_df, *args, devices=[0], **kw)
    # frames that are views: the columns of both matrices come through a permutation, the genes through a row list
    pc, ps = np.random.default_rng(6).permutation(sc_df.shape[1]), np.random.default_rng(7).permutation(S)
    sc_f = resident.DeviceFrame.from_frame(sc_df.iloc[::-1, pc]).take(np.arange(sc_df.shape[0])[::-1], np.argsort(pc))
    st_f = resident.DeviceFrame.from_frame(st_df.iloc[:, ps]).take(cols=np.argsort(ps))
    assert sc_f.columns.equals(sc_df.columns) and st_f.columns.equals(st_df.columns) and sc_f.index.equals(sc_df.index)
    resident.last_run = {"fallbacks": []}
    for a, b in ((sc_f, st_f), (sc_f, st_df), (sc_df, st_f)):
        loc, ids = apply_linear_assignment(a, b, *args, devices=[0], **kw)
        assert_frame_equal(loc, want_loc, check_exact=True)
        assert np.array_equal(ids, want_ids)
    assert sc_f.fetches == 0 and st_f.fetches == 0 and sc_f.materialized == 2 and st_f.materialized == 2
    assert resident.last_run["fallbacks"] == []
    # a launcher argument: the frames are fetched and the existing code follows
    loc, ids = apply_linear_assignment(sc_f, st_f, *args, device_id=0, **kw)
    assert_frame_equal(loc, want_loc, check_exact=True)
    assert np.array_equal(ids, want_ids)
    assert sc_f.fetches == 1 and st_f.fetches == 1 and resident.last_run["fallbacks"] == [("assign", "launcher")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ints", "dropped genes", "fractions", "square", "non-finite"])
def test_writer_writes_the_bytes_of_the_dataframe_call(case, tmp_path, hip_lib):
    G, N = 29, 44
    x = np.random.default_rng(9).poisson(0.8, (G, N)).astype(np.int64)
    if case in ("fractions", "non-finite"):
        x = x / 4.0
    if case == "non-finite":
        x[3, 5] = np.inf
    df = pd.DataFrame(x, index=[f"GENE_g{i}" for i in range(G)], columns=[f"CELL_{j}" for j in range(N)])
    cols = np.random.default_rng(10).integers(0, N, G if case == "square" else 70)
    frame = resident.DeviceFrame.from_frame(df.iloc[:, ::-1]).take(cols=np.arange(N)[::-1])     # (columns through a position list)
    if case == "dropped genes":
        keep = np.r_[0:7, 9:G]
        frame, df = frame.take(rows=keep), df.iloc[keep]
    resident.last_run = {"fallbacks": []}
    want = write_mtx_device(str(tmp_path / "host.mtx"), df, cols, return_info=True, fractions=True)
    got = write_mtx_device(str(tmp_path / "frame.mtx"), frame, cols, return_info=True, fractions=True)
    assert (tmp_path / "frame.mtx").read_bytes() == (tmp_path / "host.mtx").read_bytes()
    if case in ("square", "non-finite"):
        reason = "square" if case == "square" else "non-finite value"
        assert (want["path"], want["reason"]) == ("scipy", reason) and (got["path"], got["reason"]) == ("scipy", reason)
        assert resident.last_run["fallbacks"] == [("write_mtx", reason)] and frame.fetches == 1
    else:
        assert want["path"] == "device" and got["path"] == "device"
        assert (got["nnz"], got["bytes"], got["field"]) == (want["nnz"], want["bytes"], want["field"])
        assert frame.fetches == 0 and frame.materialized == (1 if case == "dropped genes" else 0)
        assert resident.last_run["fallbacks"] == []
