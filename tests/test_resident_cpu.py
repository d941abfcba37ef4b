"""The host half of the resident path (cytospace_amd/resident.py, csrc/select_exact.h), without a device: the "does this value
survive the conversion" predicate that cyto_select's kernel and the host hook cyto_select_check share, against numpy's round trip;
the dtype rule of DeviceFrame.narrowest against cytospace._counts_matrix; the composition of positions in DeviceFrame.take
against pandas' iloc; and the switch of main_cytospace.  Nothing has a tolerance."""
import ctypes
import inspect
import warnings

import numpy as np
import pandas as pd
import pytest

from cytospace_amd import _lib, resident
from cytospace_amd.cytospace import _counts_matrix, main_cytospace

SRC = {"int64": (np.int64, _lib.CYTO_DTYPE_I64), "float64": (np.float64, _lib.CYTO_DTYPE_F64),
       "uint16": (np.uint16, _lib.CYTO_DTYPE_U16), "float32": (np.float32, _lib.CYTO_DTYPE_F32)}
DST = dict(SRC, uint8=(np.uint8, _lib.CYTO_DTYPE_U8))
# planted: the edges of uint8 / uint16, of float32's and float64's integers, a fraction, the signed zero, the non-finite values
INTS = [-1, 0, 1, 255, 256, 65535, 65536, 2**24, 2**24 + 1, 2**53, 2**53 + 1, -(2**24) - 1, 2**62 + 1, 2**63 - 1, -(2**63)]
FLOATS = [0.5, -0.0, float("nan"), float("inf"), float("-inf"), 1e300, -1e300, 3.4028234663852886e38, 3.5e38, 0.1,
          2.0**63, -(2.0**63), 2.0**64, 65535.5, 255.0, 256.0, -1.0, 16777217.0]


def planted(src):
    if src == "int64":
        return np.array(INTS, np.int64)
    if src == "uint16":
        return np.array([0, 1, 255, 256, 65535], np.uint16)
    with np.errstate(over="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vals = np.array([float(v) for v in INTS] + FLOATS, np.float64).astype(SRC[src][0])
    return vals


def round_trip(v, dst):
    """numpy's v.astype(dst).astype(src) == v, its undefined corners settled: a non-finite value or one outside an integer
    destination's range does not survive (numpy's cast of those is undefined and platform-dependent)."""
    src = v.dtype
    ok = np.zeros(len(v), bool)
    if np.dtype(dst).kind in "iu" and src.kind == "f":
        info = np.iinfo(dst)
        # float(info.max) rounds 2^63 - 1 up to 2^63, which is out of range: compare below the next power of two
        defined = np.isfinite(v) & (v >= float(info.min)) & (v < float(2 ** (info.bits - (1 if info.min < 0 else 0))))
    else:
        defined = np.ones(len(v), bool)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = v[defined]
        ok[defined] = w.astype(dst).astype(src) == w
    return ok


def select_check(v, src, dst):
    ok = np.full(len(v), -1, np.int8)
    _lib.check(_lib.lib().cyto_select_check(v.ctypes.data, SRC[src][1], len(v), DST[dst][1], ok.ctypes.data))
    return ok.astype(bool)


@pytest.mark.parametrize("dst", sorted(DST))
@pytest.mark.parametrize("src", sorted(SRC))
def test_select_check_is_numpys_round_trip(src, dst):
    v = planted(src)
    rng = np.random.default_rng(5)
    if src in ("float64", "float32"):
        more = np.concatenate([rng.integers(-70000, 70000, 400).astype(np.float64), rng.normal(0, 300, 400),
                               rng.integers(2**23, 2**25, 200).astype(np.float64), 2.0 ** rng.integers(-30, 70, 100)])
        v = np.concatenate([v, more.astype(SRC[src][0])])
    elif src == "int64":
        v = np.concatenate([v, rng.integers(-70000, 70000, 400), rng.integers(2**52, 2**54, 200), rng.integers(2**23, 2**25, 200),
                            -rng.integers(2**23, 2**25, 200)]).astype(np.int64)
    else:
        v = np.concatenate([v, rng.integers(0, 65536, 400).astype(np.uint16)])
    v = np.ascontiguousarray(v)
    got, want = select_check(v, src, dst), round_trip(v, DST[dst][0])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(v[i], bool(got[i]), bool(want[i])) for i in bad[:10]]


def test_select_check_named_values():
    """The issue's planted values, spelt out."""
    i64 = np.array([-1, 255, 256, 65535, 65536, 2**24, 2**24 + 1, 2**53 + 1], np.int64)
    assert select_check(i64, "int64", "uint8").tolist() == [False, True, False, False, False, False, False, False]
    assert select_check(i64, "int64", "uint16").tolist() == [False, True, True, True, False, False, False, False]
    assert select_check(i64, "int64", "float32").tolist() == [True, True, True, True, True, True, False, False]
    assert select_check(i64, "int64", "float64").tolist() == [True] * 7 + [False]
    assert select_check(i64, "int64", "int64").all()
    f64 = np.array([0.5, -0.0, np.nan, np.inf, -np.inf], np.float64)
    for dst in ("uint8", "uint16", "int64"):
        assert select_check(f64, "float64", dst).tolist() == [False, True, False, False, False], dst
    for dst in ("float32", "float64"):
        assert select_check(f64, "float64", dst).tolist() == [True, True, False, True, True], dst


def test_select_check_refuses_bad_arguments():
    v, ok = np.zeros(4, np.int64), np.zeros(4, np.int8)
    L = _lib.lib()
    assert L.cyto_select_check(v.ctypes.data, _lib.CYTO_DTYPE_U8, 4, _lib.CYTO_DTYPE_I64, ok.ctypes.data) == 1     # not a source
    assert L.cyto_select_check(v.ctypes.data, _lib.CYTO_DTYPE_I64, 4, _lib.CYTO_DTYPE_I32, ok.ctypes.data) == 1    # not a destination
    assert L.cyto_select_check(None, _lib.CYTO_DTYPE_I64, 4, _lib.CYTO_DTYPE_U8, ok.ctypes.data) == 1
    assert L.cyto_select_check(v.ctypes.data, _lib.CYTO_DTYPE_I64, -1, _lib.CYTO_DTYPE_U8, ok.ctypes.data) == 1
    assert L.cyto_select_check(None, _lib.CYTO_DTYPE_I64, 0, _lib.CYTO_DTYPE_U8, None) == 0


def _range_on_host(a):
    """What cyto_value_range reports of a host array (the definition in include/cytohip.h)."""
    a = np.asarray(a)
    if a.size == 0:
        return dict(lo=np.inf, hi=-np.inf, non_integral=0, not_f32_exact=0)
    if a.dtype.kind in "iu":
        return dict(lo=int(a.min()), hi=int(a.max()), non_integral=0, not_f32_exact=0)      # (the rule for integers is lo and hi alone)
    fin = np.isfinite(a)
    with np.errstate(over="ignore"):
        a32 = a.astype(np.float32)
    return dict(lo=float(np.nanmin(a)), hi=float(np.nanmax(a)), non_integral=int(np.count_nonzero(fin & (np.trunc(a) != a))),
                not_f32_exact=int(np.count_nonzero(~np.isnan(a) & (a32.astype(np.float64) != a))))


CASES = {
    "uint8 edge": lambda r: np.r_[r.integers(0, 256, 50), 255],
    "uint8 over": lambda r: np.r_[r.integers(0, 256, 50), 256],
    "negative": lambda r: np.r_[r.integers(0, 256, 50), -1],
    "uint16 edge": lambda r: np.r_[r.integers(0, 65536, 50), 65535],
    "uint16 over": lambda r: np.r_[r.integers(0, 65536, 50), 65536],
    "float32 edge": lambda r: np.r_[r.integers(0, 2**24, 50), 2**24 - 1, -(2**24) + 1],
    "float32 over": lambda r: np.r_[r.integers(0, 2**24, 50), 2**24],
    "float32 under": lambda r: np.r_[r.integers(0, 2**24, 50), -(2**24)],
    "float64": lambda r: np.r_[r.integers(0, 2**24, 50), 2**53 + 1],
    "empty": lambda r: np.zeros(0, np.int64),
    "int32 input": lambda r: r.integers(0, 300, 40).astype(np.int32),
    "bool input": lambda r: r.integers(0, 2, 40).astype(bool),
    "floats that are float32": lambda r: r.integers(-1000, 1000, 60) / 8.0,
    "floats that are not": lambda r: np.r_[r.integers(-1000, 1000, 60) / 8.0, 0.1],
    "floats with nan": lambda r: np.r_[r.integers(-1000, 1000, 60) / 8.0, np.nan],
    "floats with nan and 0.1": lambda r: np.r_[0.1, np.nan],
    "floats with inf": lambda r: np.r_[r.integers(-1000, 1000, 60) / 8.0, np.inf, -np.inf],
    "floats beyond float32": lambda r: np.r_[1.0, 1e300],
    "float32 input": lambda r: (r.integers(-1000, 1000, 60) / 8.0).astype(np.float32),
    "uint16 input": lambda r: r.integers(0, 300, 60).astype(np.uint16),
    "uint8 input": lambda r: r.integers(0, 200, 60).astype(np.uint8),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_narrowest_dtype_is_counts_matrix(name):
    a = np.asarray(CASES[name](np.random.default_rng(11)))
    a = a.reshape(-1, 1) if a.size % 2 else a.reshape(-1, 2)
    r = _range_on_host(a)
    with np.errstate(over="ignore"):
        want = _counts_matrix(a).dtype
    assert resident.narrowest_dtype(a.dtype, r["lo"], r["hi"], r["non_integral"], r["not_f32_exact"]) == want, (name, r)


def test_take_composes_like_iloc():
    """Labels and positions alone: a frame over a buffer that does not exist (nothing here touches the device)."""
    rng = np.random.default_rng(3)
    G, C = 23, 31
    df = pd.DataFrame(np.arange(G * C).reshape(G, C), index=[f"g{i}" for i in range(G)], columns=[f"c{j}" for j in range(C)])

    class NoBuffer:
        ptr = None
    f = resident.DeviceFrame(NoBuffer(), (G, C), C, np.int64, df.index, df.columns)
    r1, c1 = rng.integers(0, G, 17), rng.permutation(C)[:19]
    r2, c2 = rng.integers(-17, 17, 40), rng.integers(-19, 19, 9)
    a = f.take(r1, c1)
    b = a.take(r2, c2)
    want1, want2 = df.iloc[r1, c1], df.iloc[r1, c1].iloc[r2, c2]
    for got, want in ((a, want1), (b, want2)):
        assert got.shape == want.shape
        assert got.index.equals(want.index) and got.columns.equals(want.columns)
        rows, cols = got.positions
        assert np.array_equal(df.to_numpy()[np.ix_(rows, cols)], want.to_numpy())
    only_rows = f.take(rows=r1)
    assert only_rows.positions[1] is None and only_rows.columns.equals(df.columns) and only_rows.index.equals(df.index[r1])
    mask = rng.integers(0, 2, C).astype(bool)
    assert f.take(cols=mask).columns.equals(df.columns[mask])
    assert f.take().positions == (None, None) and f.shape == (G, C)
    assert f.take_labels(index=["g3", "g1"], columns=["c5"]).positions[0].tolist() == [3, 1]
    with pytest.raises(KeyError):
        f.take_labels(columns=["c5", "nope"])
    with pytest.raises(IndexError):
        f.take(rows=[G])
    with pytest.raises(IndexError):
        a.take(cols=[-20])
    with pytest.raises(ValueError):
        f.columns = ["x"]
    f.columns = ["CELL_" + c for c in f.columns]
    assert f.columns[0] == "CELL_c0" and a.columns[0] == f"c{c1[0]}"      # (a view keeps the labels it was taken with)
    assert f.stats is a.stats is b.stats and f.fetches == 0 and f.materialized == 0 and f.source == "upload"
    with pytest.raises(RuntimeError):
        f.ptr


def test_main_cytospace_has_the_switch():
    p = inspect.signature(main_cytospace).parameters["resident"]
    assert p.default is None
    from cytospace_amd.cytospace import read_data
    from cytospace_amd.common import read_file_device
    assert inspect.signature(read_data).parameters["resident"].default is False
    assert inspect.signature(read_file_device).parameters["resident"].default is False


def test_check_supported_still_raises_before_any_file_is_read(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    missing = str(tmp_path / "missing.csv")
    with pytest.raises(ValueError, match="spaceranger"):
        main_cytospace(missing, missing, None, None, missing, spaceranger_path=missing, st_path=missing, coordinates_path=missing,
                       resident=True)
    with pytest.raises(ValueError, match="-ctfep"):
        main_cytospace(missing, missing, None, None, None, st_path=missing, coordinates_path=missing, resident=True)
    with pytest.raises(ValueError, match="solver_method"):
        main_cytospace(missing, missing, None, None, missing, st_path=missing, coordinates_path=missing, solver_method="lapjv",
                       resident=True)
    assert list(tmp_path.iterdir()) == []                 # (not even the output folder)


def test_new_entry_points_are_bound():
    L = _lib.lib()
    for name in ("cyto_select", "cyto_value_range", "cyto_select_check", "cyto_table_values", "cyto_table_fetch_labels",
                 "cyto_downsample_dev", "cyto_mtx_write_dev"):
        assert getattr(L, name).restype is ctypes.c_int, name
