"""write_mtx_device (csrc/mtx.hip) on the GPU against scipy.io.mmwrite(path, coo_matrix(frame.iloc[:, columns])): the same bytes,
with the default block size and with blocks forced small; every fallback with its reason and scipy's bytes; and one whole
main_cytospace run whose matrix.mtx cannot have come from scipy."""
import io
import json
import os

import numpy as np
import pandas as pd
import pytest
import scipy.io
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scipy_bytes(frame, columns):
    b = io.BytesIO()
    scipy.io.mmwrite(b, scipy.sparse.coo_matrix(frame.iloc[:, columns]))
    return b.getvalue()


def spread_values(rng, shape, dtype, density):
    """A matrix of dtype whose non-zeros run from single digits to the type's limits (the device grammar's, for the real types)."""
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
    x = np.where(rng.random(shape) < density, mag, 0).astype(dtype)
    return x


DTYPES = [np.uint8, np.uint16, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]


def shape_cases():
    """(name, frame, columns)"""
    rng = np.random.default_rng(20)
    out = []
    for dt in DTYPES:                                             # every dtype: unsorted columns with repeats, C not a multiple of 64 or 512
        x = spread_values(rng, (37, 300), dt, 0.3)
        out.append((f"{np.dtype(dt).name}_repeats", pd.DataFrame(x), rng.integers(0, 300, 1111)))
    x = spread_values(rng, (50, 40), np.int64, 0.5)
    out.append(("one_cell", pd.DataFrame(x), [17]))
    out.append(("one_gene", pd.DataFrame(x[:1]), rng.integers(0, 40, 700)))
    out.append(("one_gene_one_segment", pd.DataFrame(x[:1]), rng.integers(0, 40, 512)))
    out.append(("segment_plus_one", pd.DataFrame(x), rng.integers(0, 40, 513)))
    out.append(("wave_minus_one", pd.DataFrame(x), rng.integers(0, 40, 63)))
    z = spread_values(rng, (60, 90), np.uint16, 0.4)
    z[[0, 7, 8, 59]] = 0
    z[:, [3, 4]] = 0
    out.append(("zero_rows_and_cells", pd.DataFrame(z), np.r_[np.arange(90), 3, 4, 3]))
    out.append(("all_zero", pd.DataFrame(np.zeros((9, 30), np.int64)), np.arange(30)[::-1]))
    out.append(("all_zero_real", pd.DataFrame(np.zeros((9, 30))), np.arange(30)))
    out.append(("dense_int64_limits", pd.DataFrame(np.where(rng.random((40, 25)) < 0.5, np.iinfo(np.int64).min, np.iinfo(np.int64).max)),
                rng.integers(0, 25, 600)))
    out.append(("dense_float64_longest", pd.DataFrame(np.full((40, 25), -(2.0**53 - 1))), rng.integers(0, 25, 600)))
    out.append(("dense_uint8", pd.DataFrame(rng.integers(1, 256, (33, 64)).astype(np.uint8)), np.arange(64)))
    wide = (rng.random((3, 5000)) < 0.3) * rng.integers(1, 100000, (3, 5000))
    out.append(("six_digit_cells", pd.DataFrame(wide), rng.integers(0, 5000, 100003)))
    out.append(("labelled_frame", pd.DataFrame(x, index=[f"GENE_{i}" for i in range(50)], columns=[f"CELL_{i}" for i in range(40)]),
                [5, 5, 0, 39, 12]))
    mixed = pd.DataFrame({"a": [1, 0, 3, 0, 5], "b": [0.0, 2.0, 0.0, -40.0, 1e6], "c": [7, 0, 0, 1, 0]})
    out.append(("mixed_int_float_is_real", mixed, [1, 0, 2, 1]))
    out.append(("poisson_counts", pd.DataFrame(rng.poisson(0.1, (300, 800))), rng.integers(0, 800, 2000)))
    return out


CASES = shape_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_bytes_equal_scipys(case, tmp_path):
    from cytospace_amd.post_processing import write_mtx_device
    name, frame, columns = case
    want = scipy_bytes(frame, columns)
    p = str(tmp_path / "m.mtx")
    info = write_mtx_device(p, frame, columns, return_info=True)
    assert info["path"] == "device", info
    got = open(p, "rb").read()
    assert got == want
    assert info["bytes"] == len(want) and info["nnz"] == int(want.split(b"\n")[2].split()[2])
    assert info["field"] == want.split()[3].decode()
    assert write_mtx_device(str(tmp_path / "n.mtx"), frame.to_numpy(), columns) is None          # a plain array, no info
    assert open(str(tmp_path / "n.mtx"), "rb").read() == want


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_block_seams_leave_the_bytes_alone(case, tmp_path):
    from cytospace_amd.post_processing import write_mtx_device
    name, frame, columns = case
    want = scipy_bytes(frame, columns)
    body = len(want) - len(b"\n".join(want.split(b"\n")[:3])) - 1
    rows_with_text = int((frame.iloc[:, np.unique(columns)].to_numpy() != 0).any(axis=1).sum())
    for cap in (1, 300, max(1, body // 3)):
        p = str(tmp_path / f"m{cap}.mtx")
        info = write_mtx_device(p, frame, columns, block_bytes=cap, return_info=True)
        assert info["path"] == "device", info
        assert open(p, "rb").read() == want, cap
        if rows_with_text > 1 and cap < body:                      # (blocks are whole genes: one gene, or no text at all, is one block)
            assert info["blocks"] > 1, (cap, info)


FALLBACKS = [
    ("non-integer value", lambda x: x.__setitem__((3, 2), 2.5), np.float64),
    ("non-integer value", lambda x: x.__setitem__((3, 2), 0.1), np.float32),
    ("non-finite value", lambda x: x.__setitem__((0, 5), np.nan), np.float64),
    ("non-finite value", lambda x: x.__setitem__((11, 0), np.inf), np.float64),
    ("non-finite value", lambda x: x.__setitem__((11, 0), -np.inf), np.float32),
    ("magnitude", lambda x: x.__setitem__((6, 6), 2.0**53), np.float64),
    ("magnitude", lambda x: x.__setitem__((6, 6), -1e300), np.float64),
    ("magnitude", lambda x: x.__setitem__((6, 6), 2.0**24), np.float32),
]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(FALLBACKS)))
def test_values_outside_the_grammar_go_to_scipy(k, tmp_path, monkeypatch):
    from cytospace_amd.post_processing import write_mtx_device
    reason, poke, dt = FALLBACKS[k]
    rng = np.random.default_rng(30 + k)
    x = spread_values(rng, (12, 40), dt, 0.4)
    poke(x)
    frame, columns = pd.DataFrame(x), list(rng.integers(0, 40, 90)) + [0, 2, 5, 6]
    p = str(tmp_path / "m.mtx")
    seen = []
    real = scipy.io.mmwrite

    def watched(target, *a, **kw):
        seen.append(os.path.exists(p))                              # what the device call left at the path
        return real(target, *a, **kw)
    monkeypatch.setattr(scipy.io, "mmwrite", watched)
    open(p, "wb").write(b"stale")                                    # ... is nothing, not even what was there before
    for cap in (0, 200):
        info = write_mtx_device(p, frame, columns, block_bytes=cap, return_info=True)
        assert info["path"] == "scipy" and info["reason"] == reason, info
        assert seen[-1] is False
        assert open(p, "rb").read() == scipy_bytes(frame, columns)


@pytest.mark.gpu
def test_shapes_dtypes_and_labels_the_device_does_not_take(tmp_path):
    from cytospace_amd.post_processing import write_mtx_device
    rng = np.random.default_rng(40)
    base = rng.poisson(1.0, (20, 30))
    cases = [("square", pd.DataFrame(base), rng.integers(0, 30, 20)),
             ("dtype uint64", pd.DataFrame(base.astype(np.uint64)), [0, 1, 5]),
             ("dtype bool", pd.DataFrame(base > 0), [0, 1, 5]),
             ("duplicate labels", pd.DataFrame(base, columns=[f"c{i % 29}" for i in range(30)]), [0, 1, 2, 29])]
    for reason, frame, columns in cases:
        p = str(tmp_path / "m.mtx")
        info = write_mtx_device(p, frame, columns, return_info=True)
        assert info["path"] == "scipy" and info["reason"] == reason, info
        assert open(p, "rb").read() == scipy_bytes(frame, columns), reason
        os.remove(p)
    # the neighbours of each: the device takes them
    for frame, columns in [(pd.DataFrame(base), rng.integers(0, 30, 21)), (pd.DataFrame(base.astype(np.uint16)), [0, 1, 5])]:
        p = str(tmp_path / "d.mtx")
        assert write_mtx_device(p, frame, columns, return_info=True)["path"] == "device"
        assert open(p, "rb").read() == scipy_bytes(frame, columns)


@pytest.mark.gpu
def test_an_unwritable_path_goes_to_scipy_and_leaves_nothing(tmp_path):
    # the file cannot be created: the device call refuses ("io") and scipy gets the matrix -- whose writer, handed such a path,
    # writes nothing and raises nothing (scipy 1.15); either way nothing is at the path afterwards
    from cytospace_amd.post_processing import write_mtx_device
    p = str(tmp_path / "no_such_dir" / "m.mtx")
    x = np.arange(12).reshape(3, 4)
    try:
        scipy.io.mmwrite(p, scipy.sparse.coo_matrix(x[:, [0, 1]]))
        raised = None
    except OSError as e:
        raised = type(e)
    try:
        info = write_mtx_device(p, x, [0, 1], return_info=True)
        assert raised is None and info["path"] == "scipy" and info["reason"] == "io", info
    except OSError as e:
        assert raised is type(e)
    assert not os.path.exists(p)


@pytest.mark.gpu
def test_save_results_on_the_device_equals_the_host_path(tmp_path):
    from cytospace_amd.post_processing import save_results
    rng = np.random.default_rng(50)
    G, C = 40, 25
    expr = pd.DataFrame(rng.poisson(0.7, (G, C)), index=[f"GENE_g{i}" for i in range(G)], columns=[f"CELL_c{i}" for i in range(C)])
    ctd = pd.DataFrame({"CellType": [f"TYPE_{'ABC'[i % 3]}" for i in range(C)]}, index=expr.columns)
    coords = pd.DataFrame({"row": np.arange(9) // 3, "col": np.arange(9) % 3}, index=[f"SPOT_s{i}" for i in range(9)])
    picked = [expr.columns[i] for i in rng.integers(0, C, 31)]
    assigned = coords.iloc[rng.integers(0, 9, 31)]
    files = {}
    for tag, dev in (("host", None), ("device", 0)):
        d = tmp_path / tag
        d.mkdir()
        save_results(str(d), "p_", np.array(picked), expr, assigned, ctd, "duplicates", False, device_id=dev)
        files[tag] = {os.path.relpath(os.path.join(r, f), str(d)): open(os.path.join(r, f), "rb").read()
                      for r, _, fs in os.walk(str(d)) for f in fs}
    assert files["host"] == files["device"] and "p_assigned_expression/matrix.mtx" in files["host"]


@pytest.mark.gpu
def test_main_cytospace_writes_the_matrix_on_the_device(tmp_path, monkeypatch):
    # one whole gv14 run (unpartitioned: byte for byte) with scipy's writer made to raise: matrix.mtx is the device's
    from cytospace_amd.cytospace import main_cytospace
    gold = np.load(os.path.join(ROOT, "tests", "golden", "gv14_main.npz"))
    tag = "visium_ncpsp"
    for k in gold.files:
        if k.startswith(f"{tag}::in::"):
            (tmp_path / k.split("::")[2]).write_bytes(gold[k].tobytes())
    args = json.loads(gold[f"{tag}::args"].tobytes().decode())
    args["solver_method"] = "lapjv_hip"

    def refuse(*a, **kw):
        raise AssertionError("scipy.io.mmwrite was called")
    monkeypatch.setattr(scipy.io, "mmwrite", refuse)
    monkeypatch.chdir(tmp_path)
    main_cytospace(**args)
    out = tmp_path / args["output_folder"]
    for name in ("matrix.mtx", "genes.tsv", "barcodes.tsv"):
        assert (out / "assigned_expression" / name).read_bytes() == gold[f"{tag}::out::assigned_expression/{name}"].tobytes(), name
    assert (out / "assigned_locations.csv").read_bytes() == gold[f"{tag}::out::assigned_locations.csv"].tobytes()
