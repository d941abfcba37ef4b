"""write_csv_device / write_mtx_device with fractions=True on the GPU (csrc/csv.hip, csrc/mtx.hip, csrc/shortest.h) against the bytes
DataFrame.to_csv and scipy.io.mmwrite write for the same values at run time: at every kernel boundary (a segment is 512 cells, a
chunk 16 bytes, blocks and slabs are cut by block_bytes), with the staging buffer at its bound, on random bit patterns (the device and
the host hook share one function: a difference there is a host / device arithmetic difference), the refusals that remain, the
float64-to-float32 narrowing that fractions forbid, save_results on the device against the host branch, and poisoned work buffers."""
import os

import numpy as np
import pandas as pd
import pytest

from _text_values import mixed_matrix, pandas_bytes, random_bits, scipy_bytes

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 511), (5, 513), (7, 1025), (40, 1100)]
BLOCKS = (0, 300, 4096)
# float64 texts of 24 bytes (with their sign) in both layouts, and of one byte less
LONGEST = [-1.7976931348623157e308, -2.2250738585072014e-308, -1.2345678901234567e-100, -1.7976931348623157e-308, 1.7976931348623157e308]


def columns_for(rng, N, C):
    """C positions in [-N, N): repeats, negative positions, no order."""
    return rng.integers(-N, N, C)


def csv_device(tmp_path, x, columns, cap, **kw):
    from cytospace_amd.post_processing import write_csv_device
    p = str(tmp_path / "t.csv")
    open(p, "wb").write(b"stale, and longer than the table" * 100)
    info = write_csv_device(p, x, columns, block_bytes=cap, return_info=True, fractions=True, **kw)
    return info, open(p, "rb").read()


def mtx_device(tmp_path, x, columns, cap):
    from cytospace_amd.post_processing import write_mtx_device
    p = str(tmp_path / "m.mtx")
    open(p, "wb").write(b"stale, and longer than the matrix" * 100)
    info = write_mtx_device(p, x, columns, block_bytes=cap, return_info=True, fractions=True)
    return info, open(p, "rb").read()


def want_csv(x, columns):
    cols = np.asarray(columns)
    return pandas_bytes(x, cols, column_labels=np.where(cols < 0, cols + x.shape[1], cols))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_csv_bytes_equal_pandas(dtype, shape, tmp_path):
    G, C = shape
    rng = np.random.default_rng(G * C)
    N = max(3, C // 2 + 7)                                         # fewer source columns than cells: repeats
    x = mixed_matrix(dtype, G, N, seed=G + C)
    columns = columns_for(rng, N, C)
    want = want_csv(x, columns)
    assert C == 1 or (b"e-" in want and b"e+" in want and b".0," in want and b"-0.0" in want)
    for cap in BLOCKS:
        info, got = csv_device(tmp_path, x, columns, cap)
        assert info["path"] == "device", info
        assert got == want, cap
        assert info["bytes"] == len(want)
        assert info["blocks"] > 1 or cap == 0 or G == 1            # (a gene's text, at 20 or 25 bytes a field, is above either cap)
    # default arguments: the same matrix goes to pandas
    from cytospace_amd.post_processing import write_csv_device
    info = write_csv_device(str(tmp_path / "d.csv"), x, columns, return_info=True)
    assert info["path"] == "pandas" or C == 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_mtx_bytes_equal_scipy(dtype, shape, tmp_path):
    G, C = shape
    if G == C:                                                     # (a square result is scipy's: one gene more)
        G += 1
    rng = np.random.default_rng(G * C + 1)
    N = max(3, C // 2 + 7)
    x = mixed_matrix(dtype, G, N, seed=G + C + 1, zeros=0.5)
    columns = columns_for(rng, N, C)
    want = scipy_bytes(x, np.where(columns < 0, columns + N, columns))
    nnz = int(np.count_nonzero(x[:, columns]))
    for cap in BLOCKS:
        info, got = mtx_device(tmp_path, x, columns, cap)
        assert info["path"] == "device", info
        assert got == want, cap
        assert info["nnz"] == nnz and info["field"] == "real" and info["bytes"] == len(want)
        assert f"\n{G} {C} {nnz}\n".encode() in got[:200]


@pytest.mark.parametrize("C", [512, 1024])
def test_staging_buffer_at_its_bound_and_at_its_emptiest(C, tmp_path):
    # every value of a segment at the longest text: the segment fills the LDS staging buffer to its last byte; then one character each
    rng = np.random.default_rng(C)
    G = 5
    for name, pool, dtype in (("longest float64", LONGEST[:4], np.float64), ("longest float32", [-9999999000000000.0, -1.2345679e-05], np.float32),
                              ("one character", [1.0, 2.0, 7.0], np.float64)):
        x = np.array(pool, dtype)[rng.integers(0, len(pool), (G, C))]
        if name == "one character":
            xi = x.astype(np.uint8)                                # "7": the shortest field and line there is
            columns = np.arange(C)
            for cap in (0, 4096):
                info, got = csv_device(tmp_path, xi, columns, cap)
                assert info["path"] == "device" and got == want_csv(xi, columns), (name, cap)
        columns = np.arange(C)[::-1].copy()
        want_c, want_m = want_csv(x, columns), scipy_bytes(x, columns)
        if name == "longest float64":
            longest = max(len(f) for f in want_c.split(b"\n")[1].split(b",")[1:])
            assert longest == 24 and max(len(l.split(b" ")[2]) for l in want_m.split(b"\n")[3:-1]) == 24
        for cap in (0, 300, 4096):
            info, got = csv_device(tmp_path, x, columns, cap)
            assert info["path"] == "device" and got == want_c, (name, cap)
            info, got = mtx_device(tmp_path, x, columns, cap)
            assert info["path"] == "device" and got == want_m, (name, cap)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_device_equals_the_host_function_on_random_bit_patterns(dtype, tmp_path):
    G, C = 300, 1100
    v = random_bits(dtype, G * C + 20000, seed=77)[:G * C]         # (the non-finite patterns are dropped, not replaced by one value)
    assert len(v) == G * C
    x = np.ascontiguousarray(v.reshape(G, C))
    columns = np.arange(C)
    info, got = csv_device(tmp_path, x, columns, 0)
    assert info["path"] == "device"
    assert got == want_csv(x, columns)
    info, got = mtx_device(tmp_path, x, columns, 0)
    assert info["path"] == "device" and info["nnz"] == np.count_nonzero(x)
    assert got == scipy_bytes(x)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_in_the_last_slab_still_goes_to_the_library(bad, tmp_path, monkeypatch):
    import scipy.io
    x = mixed_matrix(np.float64, 12, 40, seed=3, zeros=0.3)
    x[11, 2] = bad
    columns = np.r_[np.arange(40), 2, 2]
    seen = []
    real_csv, real_mm = pd.DataFrame.to_csv, scipy.io.mmwrite

    def to_csv(self, target=None, *a, **kw):
        seen.append(("csv", os.path.exists(str(target))))          # what the device call left at the path
        return real_csv(self, target, *a, **kw)

    def mmwrite(target, *a, **kw):
        seen.append(("mtx", os.path.exists(str(target))))
        return real_mm(target, *a, **kw)
    want_c, want_m = want_csv(x, columns), scipy_bytes(x, columns)
    monkeypatch.setattr(pd.DataFrame, "to_csv", to_csv)
    monkeypatch.setattr(scipy.io, "mmwrite", mmwrite)
    for cap in (0, 200):                                           # one slab; a gene or so per slab: the partial file goes
        info, got = csv_device(tmp_path, x, columns, cap)
        assert info["path"] == "pandas" and info["reason"] == "non-finite value", info
        assert seen[-1] == ("csv", False) and got == want_c
        info, got = mtx_device(tmp_path, x, columns, cap)
        assert info["path"] == "scipy" and info["reason"] == "non-finite value", info
        assert seen[-1] == ("mtx", False) and got == want_m
    assert len(seen) == 4


def test_a_float64_frame_of_float32_exact_fractions_keeps_float64s_digits(tmp_path):
    rng = np.random.default_rng(8)
    x = np.where(rng.random((9, 30)) < 0.5, 0.5, np.float32(0.1).astype(np.float64))
    x[rng.random((9, 30)) < 0.3] = 0
    assert np.array_equal(x.astype(np.float32), x)                 # float32-exact: the default path's narrowing test passes
    columns = rng.integers(0, 30, 70)
    for m in (x, pd.DataFrame(x)):
        info, got = mtx_device(tmp_path, m, columns, 0)
        assert info["path"] == "device"
        assert got == scipy_bytes(x, columns) and b"1.0000000149011612E-1" in got and b" 5E-1\n" in got


def _files(d):
    return {os.path.relpath(os.path.join(r, f), str(d)): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(str(d)) for f in fs}


@pytest.mark.parametrize("method", ["duplicates", "place_holders"])
def test_save_results_on_the_device_equals_the_host_branch_on_a_fractional_frame(method, tmp_path, monkeypatch):
    from cytospace_amd import post_processing
    rng = np.random.default_rng(50)
    G, C, P = 30, 25, 9
    cells = [f"CELL_c{i}" for i in range(C)]
    new = [f"CELL_{'ABC'[k % 3]}_new_{k + 1}" for k in range(P)] if method == "place_holders" else []
    expr = pd.DataFrame(mixed_matrix(np.float64, G, C + len(new), seed=9, zeros=0.4), index=[f"GENE_g{i}" for i in range(G)], columns=cells + new)
    ctd = pd.DataFrame({"CellType": [f"TYPE_{'ABC'[i % 3]}" for i in range(C)]}, index=cells)
    coords = pd.DataFrame({"row": np.arange(9) // 3, "col": np.arange(9) % 3}, index=[f"SPOT_s{i}" for i in range(9)])
    picked = [cells[i] for i in rng.integers(0, C, 60 - len(new))] + new            # 60 assigned cells, 30 genes
    assigned = coords.iloc[rng.integers(0, 9, 60)]
    infos = []
    for name in ("write_mtx_device", "write_csv_device"):
        def wrapper(*a, _real=getattr(post_processing, name), _name=name, **kw):
            info = _real(*a, return_info=True, **kw)
            infos.append((_name, info["path"], info.get("reason")))
        monkeypatch.setattr(post_processing, name, wrapper)
    files = {}
    for tag, dev in (("host", None), ("device", 0)):
        d = tmp_path / tag
        d.mkdir()
        post_processing.save_results(str(d), "p_", np.array(picked), expr, assigned, ctd, method, False, device_id=dev)
        files[tag] = _files(d)
    assert infos == [("write_mtx_device" if method == "duplicates" else "write_csv_device", "device", None)]
    assert files["host"] == files["device"]
    big = files["device"]["p_assigned_expression/matrix.mtx" if method == "duplicates" else "p_new_scRNA.csv"]
    assert (b"E-" in big) if method == "duplicates" else (b"e-" in big)                 # fractional text went through


@pytest.mark.parametrize("writer", ["csv", "mtx"])
def test_poisoned_work_buffers_leave_the_bytes_alone(writer, tmp_path):
    from cytospace_amd import _lib
    rng = np.random.default_rng(21)
    x = mixed_matrix(np.float64, 37, 300, seed=21, zeros=0.3)
    columns = rng.integers(0, 300, 1111)
    want = want_csv(x, columns) if writer == "csv" else scipy_bytes(x, columns)
    device = csv_device if writer == "csv" else mtx_device
    try:
        for byte in (0x00, 0xFF, 0x7F, 0xA5):
            _lib.cache_poison(byte)
            for blocks in ("fresh", "reused"):
                if blocks == "fresh":
                    _lib.trim_device_cache()
                fills = _lib.cache_poison_fills()
                info, got = device(tmp_path, x, columns, 300)
                assert info["path"] == "device" and info["blocks"] > 1, info
                assert got == want, (hex(byte), blocks)
                assert _lib.cache_poison_fills() > fills
    finally:
        _lib.cache_poison(None)
        _lib.trim_device_cache()
