"""write_csv_device (csrc/csv.hip) on the GPU against DataFrame.to_csv of the selected, relabelled frame: the same bytes, with the
default slab size and with slabs forced small; every fallback with its reason and pandas' bytes; save_results with place-holders on
the device against the host branch and the reference's own file; and one whole main_cytospace run whose new_scRNA.csv cannot have
come from pandas."""
import io
import json
import os

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.uint8, np.uint16, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]


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


def spread_values(rng, shape, dtype, density=0.7):
    """A matrix of dtype whose values run from zero and single digits to the type's limits (the device grammar's, for the real types)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        top, signed = (2**24 - 1, True) if dtype == np.float32 else (2**53 - 1, True)
    else:
        ii = np.iinfo(dtype)
        top, signed = ii.max, ii.min < 0
    bits = rng.integers(1, int(top).bit_length(), shape, endpoint=True)
    mag = (rng.integers(0, 2**62, shape) % (np.int64(1) << bits.astype(np.int64).clip(max=62))).astype(np.int64)
    mag = np.where(rng.random(shape) < 0.1, top, np.minimum(mag, top))           # the limit itself, often
    mag = np.where(rng.random(shape) < 0.2, (mag // 1000) * 1000, mag)             # trailing zeros
    if signed:
        mag = np.where(rng.random(shape) < 0.4, -mag, mag)
        if dtype.kind == "i":
            mag = np.where(rng.random(shape) < 0.05, np.iinfo(dtype).min, mag)
    return np.where(rng.random(shape) < density, mag, 0).astype(dtype)


# gene labels of 0, 1, 15, 16, 17 and 300 bytes (row starts at every alignment), and those that pandas quotes
LABELS = ["", "g", "fifteen_bytes_1", "sixteen_bytes_16", "seventeen_bytes_1", "L" * 300, "with,comma", 'with"quote', "with\nnewline",
          " leading space", "gène_µ_細胞", "", "x" * 15, "y" * 16, "z" * 17, "w" * 299 + ","]
assert [len(s.encode()) for s in LABELS[:6]] == [0, 1, 15, 16, 17, 300]


def shape_cases():
    """(name, frame or array, columns, keyword arguments)"""
    rng = np.random.default_rng(20)
    out = []
    for dt in DTYPES:                                             # every dtype: unsorted columns with repeats, C not a multiple of 64 or 512
        x = spread_values(rng, (37, 300), dt)
        out.append((f"{np.dtype(dt).name}_repeats", pd.DataFrame(x), rng.integers(0, 300, 1111), {}))
    x = spread_values(rng, (50, 40), np.int64)
    xf = spread_values(rng, (50, 40), np.float64)
    for C in (1, 63, 512, 513, 1025):                            # a cell, a wave less one, a segment, one more, two and one more
        out.append((f"int64_C{C}", pd.DataFrame(x), rng.integers(0, 40, C), {}))
        out.append((f"float64_C{C}", pd.DataFrame(xf), rng.integers(0, 40, C), {}))
    out.append(("one_gene", pd.DataFrame(xf[:1]), rng.integers(0, 40, 700), {}))
    out.append(("one_gene_one_cell", pd.DataFrame(x[:1]), [-1], {}))
    for dt in DTYPES:
        out.append((f"all_zero_{np.dtype(dt).name}", pd.DataFrame(np.zeros((9, 30), dt)), np.arange(30)[::-1], {}))
    for dt in (np.float32, np.float64):
        z = spread_values(rng, (20, 33), dt)
        z[rng.random(z.shape) < 0.3] = -0.0
        z[:, 4] = -0.0
        z[7] = -0.0
        assert np.signbit(z[7]).all()
        out.append((f"negative_zeros_{np.dtype(dt).name}", pd.DataFrame(z), np.r_[np.arange(33), 4, 4, rng.integers(0, 33, 600)], {}))
    out.append(("longest_float64", pd.DataFrame(np.full((40, 25), -(2.0**53 - 1))), rng.integers(0, 25, 600), {}))
    out.append(("longest_float32", pd.DataFrame(np.full((40, 25), -(2.0**24 - 1), np.float32)), rng.integers(0, 25, 600), {}))
    out.append(("longest_int64", pd.DataFrame(np.full((40, 25), np.iinfo(np.int64).min)), rng.integers(0, 25, 1024), {}))
    out.append(("plain_array", spread_values(rng, (21, 50), np.int32), rng.integers(-50, 50, 200), {}))
    out.append(("plain_array_float32", spread_values(rng, (21, 50), np.float32), rng.integers(-50, 50, 200), {}))
    xl = spread_values(rng, (len(LABELS), 70), np.float64)
    out.append(("label_lengths", pd.DataFrame(xl, index=LABELS), rng.integers(0, 70, 530), {}))
    out.append(("label_lengths_one_cell", pd.DataFrame(spread_values(rng, (len(LABELS), 70), np.int16), index=LABELS[::-1]), [3], {}))
    out.append(("given_labels_and_name", pd.DataFrame(x), [5, 5, 0, 39, 12],
                dict(index_labels=(LABELS * 4)[:50], column_labels=["a", "b,c", "", 'q"', "a"], index_name="Gene, name")))
    named = pd.DataFrame(x, index=pd.Index([f"GENE_{i}" for i in range(50)], name="genes"), columns=[f"CELL_{i}" for i in range(40)])
    out.append(("frames_own_labels_and_name", named, [5, 5, 0, 39, 12], {}))
    mixed = pd.DataFrame({"a": [1, 0, 3, 0, 5], "b": [0.0, 2.0, -0.0, -40.0, 1e6], "c": [7, 0, 0, 1, 0], "d": [1.0, 2.0, 3.0, 4.0, 5.0]})
    out.append(("float_columns_of_a_mixed_frame", mixed, [3, 1, 1], {}))
    out.append(("int_columns_of_a_mixed_frame", mixed, [2, 0, 2], {}))
    out.append(("poisson_counts", pd.DataFrame(rng.poisson(0.5, (300, 800)).astype(np.float64)), rng.integers(0, 800, 2000), {}))
    return out


CASES = shape_cases()
WANT = {}


def want_bytes(case):
    """pandas' bytes for the case, computed once."""
    name, m, columns, kw = case
    if name not in WANT:
        if isinstance(m, pd.DataFrame):
            WANT[name] = pandas_bytes(m, columns, **kw)
        else:
            cols = np.asarray(columns)
            WANT[name] = pandas_bytes(pd.DataFrame(m), columns, column_labels=np.where(cols < 0, cols + m.shape[1], cols))
    return WANT[name]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_bytes_equal_pandas(case, tmp_path):
    from cytospace_amd.post_processing import write_csv_device
    name, m, columns, kw = case
    want = want_bytes(case)
    p = str(tmp_path / "t.csv")
    open(p, "wb").write(b"stale, and longer than the table" * 2000)
    info = write_csv_device(p, m, columns, return_info=True, **kw)
    assert info["path"] == "device", info
    got = open(p, "rb").read()
    assert got == want
    assert info["bytes"] == len(want) and info["blocks"] >= 1
    assert write_csv_device(str(tmp_path / "n.csv"), m, columns, **kw) is None          # no info
    assert open(str(tmp_path / "n.csv"), "rb").read() == want


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_slab_seams_leave_the_bytes_alone(case, tmp_path):
    from cytospace_amd.post_processing import write_csv_device
    name, m, columns, kw = case
    want = want_bytes(case)
    body = len(want) - want.index(b"\n") - 1                      # (no case has a line end in its header)
    for cap in (1, 300, max(1, body // 3)):
        p = str(tmp_path / f"t{cap}.csv")
        info = write_csv_device(p, m, columns, block_bytes=cap, return_info=True, **kw)
        assert info["path"] == "device", info
        assert open(p, "rb").read() == want, cap
        if m.shape[0] > 1:                                         # (slabs are whole genes: one gene is one slab)
            assert info["blocks"] > 1, (cap, info)
        else:
            assert info["blocks"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("byte", [0xFF, 0x7F])
def test_poisoned_work_buffers_leave_the_bytes_alone(byte, tmp_path):
    # every device buffer of the call arrives filled with the byte (0xFF: NaN words, huge offsets): nothing is read before it is written
    from cytospace_amd import _lib
    from cytospace_amd.post_processing import write_csv_device
    case = next(c for c in CASES if c[0] == "label_lengths")
    fills = _lib.cache_poison_fills()
    _lib.cache_poison(byte)
    try:
        for cap in (0, 300):
            p = str(tmp_path / f"t{cap}.csv")
            assert write_csv_device(p, case[1], case[2], block_bytes=cap, return_info=True)["path"] == "device"
            assert open(p, "rb").read() == want_bytes(case)
    finally:
        _lib.cache_poison(None)
    assert _lib.cache_poison_fills() > fills


# (reason, the offending value, dtype)
REFUSED = [("non-integer value", 2.5, np.float64), ("non-integer value", 0.1, np.float32), ("non-integer value", -1e-300, np.float64),
           ("non-finite value", np.nan, np.float64), ("non-finite value", np.inf, np.float64), ("non-finite value", -np.inf, np.float32),
           ("non-finite value", np.nan, np.float32),
           ("magnitude", 2.0**53, np.float64), ("magnitude", -1e300, np.float64), ("magnitude", 2.0**24, np.float32),
           ("magnitude", -(2.0**24), np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_values_outside_the_grammar_go_to_pandas(k, tmp_path, monkeypatch):
    from cytospace_amd.post_processing import write_csv_device
    reason, value, dt = REFUSED[k]
    rng = np.random.default_rng(30 + k)
    p = str(tmp_path / "t.csv")
    seen = []
    real = pd.DataFrame.to_csv

    def watched(self, target=None, *a, **kw):
        if target == p:
            seen.append(os.path.exists(p))                          # what the device call left at the path
        return real(self, target, *a, **kw)
    monkeypatch.setattr(pd.DataFrame, "to_csv", watched)
    for where in ((0, 5), (11, 2)):                                  # in the first slab and in the last
        x = spread_values(rng, (12, 40), dt)
        x[where] = value
        frame, columns = pd.DataFrame(x), list(rng.integers(0, 40, 90)) + [0, 2, 5, 6]
        want = pandas_bytes(frame, columns)
        for cap in (0, 200):                                         # one slab; a gene per slab: the partial file goes
            open(p, "wb").write(b"stale")
            info = write_csv_device(p, frame, columns, block_bytes=cap, return_info=True)
            assert info["path"] == "pandas" and info["reason"] == reason, info
            assert seen[-1] is False
            assert open(p, "rb").read() == want
    assert len(seen) == 4


@pytest.mark.gpu
def test_frames_the_device_does_not_take_and_their_neighbours(tmp_path, monkeypatch):
    from cytospace_amd.post_processing import write_csv_device
    rng = np.random.default_rng(40)
    base = rng.poisson(1.0, (20, 30))
    p = str(tmp_path / "t.csv")
    seen = []
    real = pd.DataFrame.to_csv

    def watched(self, target=None, *a, **kw):
        if target == p:
            seen.append(os.path.exists(p))
        return real(self, target, *a, **kw)
    monkeypatch.setattr(pd.DataFrame, "to_csv", watched)
    mixed = pd.DataFrame(base).astype({3: np.float64})
    cases = [("dtype uint64", pd.DataFrame(base.astype(np.uint64)), [0, 1, 5]),
             ("dtype bool", pd.DataFrame(base > 0), [0, 1, 5]),
             ("dtype float16", pd.DataFrame(base.astype(np.float16)), [0, 1, 5]),
             ("mixed dtypes", mixed, [0, 3, 5]),
             ("duplicate labels", pd.DataFrame(base, columns=[f"c{i % 29}" for i in range(30)]), [0, 1, 2, 29]),
             ("empty", pd.DataFrame(base), []),
             ("empty", pd.DataFrame(base[:0]), [0, 1])]
    for reason, frame, columns in cases:
        open(p, "wb").write(b"stale")
        info = write_csv_device(p, frame, columns, return_info=True)
        assert info["path"] == "pandas" and info["reason"] == reason, info
        assert seen[-1] is False, reason
        assert open(p, "rb").read() == pandas_bytes(frame, columns), reason
    n = len(seen)
    buf = io.StringIO()
    assert write_csv_device(buf, pd.DataFrame(base), [0, 1], return_info=True)["reason"] == "not a path"
    assert buf.getvalue().encode() == pandas_bytes(pd.DataFrame(base), [0, 1])
    # the neighbours of each: the device takes them
    edge = np.full((20, 30), 2.0**53 - 1)
    edge32 = np.full((20, 30), 2.0**24 - 1, np.float32)
    for frame, columns in [(pd.DataFrame(base.astype(np.uint16)), [0, 1, 5]), (pd.DataFrame(base.astype(np.int8)), [0, 1, 5]),
                           (mixed, [0, 4, 5]), (mixed, [3, 3]), (pd.DataFrame(edge), [0, 1, 5]), (pd.DataFrame(-edge), [7]),
                           (pd.DataFrame(edge32), [0, 1, 5]), (pd.DataFrame(base[:1]), [0]),
                           (pd.DataFrame(base, columns=[f"c{i}" for i in range(30)], index=["g"] * 20), [0, 1, 2, 29])]:
        assert write_csv_device(p, frame, columns, return_info=True)["path"] == "device"
        assert open(p, "rb").read() == pandas_bytes(frame, columns)
    assert len(seen) == n


@pytest.mark.gpu
def test_an_unwritable_path_goes_to_pandas_and_leaves_nothing(tmp_path, monkeypatch):
    # the file cannot be created: the device call refuses ("io") and pandas gets the frame -- and raises what it raises for such a path
    from cytospace_amd.post_processing import write_csv_device
    p = str(tmp_path / "no_such_dir" / "t.csv")
    x = np.arange(12).reshape(3, 4)
    reasons = []
    real = pd.DataFrame.to_csv

    def watched(self, target=None, *a, **kw):
        reasons.append(target)
        return real(self, target, *a, **kw)
    monkeypatch.setattr(pd.DataFrame, "to_csv", watched)
    with pytest.raises(OSError):
        write_csv_device(p, x, [0, 1], return_info=True)
    assert reasons == [p] and not os.path.exists(p)
    # a directory in the file's place: open() fails after the checks, nothing of the device's is left, pandas raises
    d = tmp_path / "dir.csv"
    d.mkdir()
    with pytest.raises(OSError):
        write_csv_device(str(d), x, [0, 1])
    assert reasons[-1] == str(d) and os.path.isdir(str(d))


def _files(d):
    return {os.path.relpath(os.path.join(r, f), str(d)): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(str(d)) for f in fs}


@pytest.mark.gpu
def test_save_results_place_holders_on_the_device_equals_the_host_path(tmp_path, monkeypatch):
    # a float frame whose index has a name, as read_file's frames have: the host branch drops the name, so does the device branch;
    # and on the device leg pandas must not be the one that writes new_scRNA.csv
    from cytospace_amd.post_processing import save_results
    rng = np.random.default_rng(50)
    G, C, P = 40, 25, 9
    cells = [f"CELL_c{i}" for i in range(C)]
    new = [f"CELL_{'ABC'[k % 3]}_new_{k + 1}" for k in range(P)]
    expr = pd.DataFrame(rng.poisson(0.7, (G, C + P)).astype(np.float64), index=pd.Index([f"GENE_g{i}" for i in range(G)], name="GENES"),
                        columns=cells + new)
    expr.iloc[3, C + 2] = -0.0
    ctd = pd.DataFrame({"CellType": [f"TYPE_{'ABC'[i % 3]}" for i in range(C)]}, index=cells)
    coords = pd.DataFrame({"row": np.arange(9) // 3, "col": np.arange(9) % 3}, index=[f"SPOT_s{i}" for i in range(9)])
    picked = [cells[i] for i in rng.integers(0, C, 22)] + new
    assigned = coords.iloc[rng.integers(0, 9, 31)]
    real = pd.DataFrame.to_csv
    leg = []

    def watched(self, target=None, *a, **kw):
        assert leg[-1] == "host" or not str(target).endswith("new_scRNA.csv"), "pandas wrote new_scRNA.csv on the device leg"
        return real(self, target, *a, **kw)
    monkeypatch.setattr(pd.DataFrame, "to_csv", watched)
    files = {}
    for tag, dev in (("host", None), ("device", 0)):
        leg.append(tag)
        d = tmp_path / tag
        d.mkdir()
        save_results(str(d), "p_", np.array(picked), expr, assigned, ctd, "place_holders", False, device_id=dev)
        files[tag] = _files(d)
    assert files["host"] == files["device"] and files["host"]["p_new_scRNA.csv"].startswith(b",A_new_1,B_new_2,C_new_3,")
    assert b"-0.0" in files["device"]["p_new_scRNA.csv"] and expr.index.name == "GENES"


@pytest.mark.gpu
@pytest.mark.parametrize("single", [False, True])
def test_save_results_writes_the_references_new_scrna_on_the_device(single, tmp_path, monkeypatch):
    # the gv12 toy inputs (an int frame; tests/test_abi_cpu.py builds the same): the file the reference wrote, and not from pandas
    from cytospace_amd.post_processing import save_results
    gold = np.load(os.path.join(ROOT, "tests", "golden", "gv12_outputs.npz"))
    rng = np.random.default_rng(12)
    G, C, S = 7, 14, 6
    cells = [f"CELL_c{i}" for i in range(C)]
    types_ = ["TYPE_B", "TYPE_T", "TYPE_Mono"]
    ctd = pd.DataFrame({"CellType": [types_[i % 3] for i in range(C)]}, index=cells)
    expr = pd.DataFrame(rng.poisson(2.0, (G, C)), index=[f"GENE_g{i}" for i in range(G)], columns=cells)
    coords = pd.DataFrame({"row": np.arange(S) // 3, "col": np.arange(S) % 3}, index=[f"SPOT_s{i}" for i in range(S)])
    picked = [cells[i] for i in (3, 0, 7, 7, 12, 5, 9, 1, 3, 13, 2)]
    extra = [f"CELL_{t[5:]}_new_{k + 1}" for k, t in enumerate(["TYPE_B", "TYPE_Mono"])]
    for e in extra:
        expr[e] = rng.poisson(2.0, G)
    picked = picked[:9] + extra
    assigned = coords.loc[[coords.index[i] for i in (0, 0, 1, 3, 3, 3, 4, 1, 0, 4, 3)]]
    real = pd.DataFrame.to_csv

    def watched(self, target=None, *a, **kw):
        assert not str(target).endswith("new_scRNA.csv"), "pandas wrote new_scRNA.csv"
        return real(self, target, *a, **kw)
    monkeypatch.setattr(pd.DataFrame, "to_csv", watched)
    save_results(str(tmp_path), "p_", np.array(picked), expr, assigned, ctd, "place_holders", single, device_id=0)
    tag = f"place_holders_{'sc' if single else 'spot'}"
    got = _files(tmp_path)
    want = {k.split("::", 1)[1]: bytes(gold[k].tobytes()) for k in gold.files if k.startswith(tag + "::")}
    want.pop("p_unassigned_locations.csv", None)                    # (save_unassigned_locations' file)
    assert got == want and got["p_new_scRNA.csv"].startswith(b",B_new_1,Mono_new_2\ng0,")


@pytest.mark.gpu
def test_main_cytospace_writes_the_place_holder_table_on_the_device(tmp_path, monkeypatch):
    # one whole gv14 run (unpartitioned: byte for byte) with pandas' writer made to raise for new_scRNA.csv: the file is the device's
    from cytospace_amd.cytospace import main_cytospace
    gold = np.load(os.path.join(ROOT, "tests", "golden", "gv14_main.npz"))
    tag = "estimated_placeholders"
    for k in gold.files:
        if k.startswith(f"{tag}::in::"):
            (tmp_path / k.split("::")[2]).write_bytes(gold[k].tobytes())
    args = json.loads(gold[f"{tag}::args"].tobytes().decode())
    args["solver_method"] = "lapjv_hip"
    real = pd.DataFrame.to_csv

    def watched(self, target=None, *a, **kw):
        if str(target).endswith("new_scRNA.csv"):
            raise AssertionError("DataFrame.to_csv was called for new_scRNA.csv")
        return real(self, target, *a, **kw)
    monkeypatch.setattr(pd.DataFrame, "to_csv", watched)
    monkeypatch.chdir(tmp_path)
    main_cytospace(**args)
    out = tmp_path / args["output_folder"]
    for name in ("new_scRNA.csv", "assigned_locations.csv"):
        assert (out / name).read_bytes() == gold[f"{tag}::out::{name}"].tobytes(), name
