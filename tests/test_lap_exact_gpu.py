"""cyto_lap_opts.exact: the float32 solve repaired on its near-tight edges E = {(i, j) : r_ij <= tau} (include/cytohip.h; DESIGN.md,
"Exact option") -- the optimum of the float32 matrix, whatever the float32 solver's constants."""
import hashlib

import numpy as np
import pytest

from cytospace_amd import _lib
from cytospace_amd.lap import lap_solve, lap_solve_batch, lap_solve_rows, lapjv_hip
from oracle.jv import jv_oracle

pytestmark = pytest.mark.gpu


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def _opt(c):
    from scipy.optimize import linear_sum_assignment
    c64 = np.asarray(c, np.float64)
    r, cc = linear_sum_assignment(c64)
    return float(c64[r, cc].sum())


def _near_tight(c, rowsol, v, gap):
    """E recomputed in numpy with the kernel's operations (tau as include/cytohip.h writes it): per row the count of j != rowsol[i]"""
    n = len(c)
    ar = np.arange(n)
    w = np.asarray(c, np.float64) - np.asarray(v, np.float64)[None, :]
    r = w - w[ar, rowsol][:, None]
    E = r <= gap * (1.0 + 2.0 ** -30)
    E[ar, rowsol] = False
    return E.sum(1)


def _certificate(c, rowsol, v):
    n = len(c)
    w = np.asarray(c, np.float64) - np.asarray(v, np.float64)[None, :]
    return float(np.maximum(w[np.arange(n), rowsol] - w.min(1), 0.0).sum())


def _i283():
    from tools import cross_unique
    return cross_unique.instance("typed", 2973, 5283, 4)


def _additive(n):
    # c_ij = fl32(x_i + y_j): every permutation costs the same up to the rounding of the sums -- nearly every edge is near-tight
    rng = np.random.default_rng(n)
    x, y = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
    return (x[:, None] + y[None, :]).astype(np.float32)


def test_exact_gives_the_golden_indices_on_every_certified_unique_instance():
    from tools import cross_unique
    d = np.load(cross_unique.OUT)
    m = len(d["n"])
    assert m >= 300
    bad = []
    for k in range(m):
        c = cross_unique.instance(str(d["kind"][k]), int(d["n"][k]), int(d["seed"][k]), int(d["K"][k]))
        for opts in ((dict(exact=1),) + ((dict(exact=1, mode=1),) if k < 20 else ())):
            g = lap_solve(c, np.float32, return_info=True, opts=opts)
            i = g["info"]
            assert i.certified == 1 and i.exact_status in (1, 2), (k, opts)
            if _sha(g["colsol"]) != str(d["colsol_sha256"][k]):
                bad.append((k, opts))
    assert not bad, bad


def test_exact_recovers_the_unique_optimum_of_instance_283():
    c = _i283()
    n = len(c)
    g = lap_solve(c, np.float32, return_info=True, opts=dict(exact=1))
    i = g["info"]
    assert i.exact_status == 2 and i.exact_changed_rows > 0 and i.exact_free_rows == i.gap_rows > 0 and i.polished == 0
    o = jv_oracle(c, np.float32)
    assert np.array_equal(g["rowsol"], o["rowsol"]) and np.array_equal(g["colsol"], o["colsol"])
    p = lap_solve(c, np.float32, return_info=True, opts=dict(polish=1))
    assert np.array_equal(g["rowsol"], p["rowsol"]) and np.array_equal(g["colsol"], p["colsol"])
    opt = _opt(c)
    assert abs(g["total"] - opt) <= 1e-12 * abs(opt)
    assert abs(float(c.astype(np.float64)[np.arange(n), g["rowsol"]].sum()) - opt) <= 1e-12 * abs(opt)
    # v is the float32 solve's; a changed row's u is fl32(c - v) on its new column
    b = lap_solve(c, np.float32, return_info=True, opts=dict(certify=1))
    assert np.array_equal(g["v"], b["v"])
    moved = g["rowsol"] != b["rowsol"]
    assert int(moved.sum()) == i.exact_changed_rows
    assert np.array_equal(g["u"][moved], c[np.flatnonzero(moved), g["rowsol"][moved]] - g["v"][g["rowsol"][moved]])
    assert np.array_equal(g["u"][~moved], b["u"][~moved])
    # the lapjv-shaped entry point
    row_ind, col_ind, (total, u, v) = lapjv_hip(c, exact=True)
    assert np.array_equal(row_ind, o["rowsol"]) and np.array_equal(col_ind, o["colsol"]) and total == g["total"]


def _check_edges(c, solve):
    b = solve(dict(certify=1))
    g = solve(dict(exact=1))
    bi, gi = b["info"], g["info"]
    assert gi.gap_f64 == bi.gap_f64 and gi.gap_rows == bi.gap_rows and np.array_equal(g["v"], b["v"])
    cnt = _near_tight(c, b["rowsol"], b["v"], bi.gap_f64)
    assert gi.exact_status == (2 if bi.gap_f64 > 0 else 1)
    assert gi.exact_edges == (int(cnt.sum()) if bi.gap_f64 > 0 else 0)
    assert gi.exact_free_rows == (bi.gap_rows if bi.gap_f64 > 0 else 0)
    assert gi.exact_overflow_rows == (int((cnt > 16).sum()) if bi.gap_f64 > 0 else 0)
    assert _certificate(c, g["rowsol"], g["v"]) <= bi.gap_f64
    opt = _opt(c)
    assert abs(g["total"] - opt) <= 1e-12 * max(1.0, abs(opt))
    return g


def test_exact_edges_match_numpy():
    from tools import instances
    for c in (np.random.default_rng(41).random((1500, 1500)).astype(np.float32), instances.typed_unique_cost(2003, 2003, 9)[0]):
        g = _check_edges(c, lambda o: lap_solve(c, np.float32, return_info=True, opts=o))
        assert g["info"].gap_f64 > 0
    # a row map: the same E as the materialised matrix
    rows = instances.typed_unique_cost(300, 1200, 11)[0]
    rowmap = np.repeat(np.arange(300), 4).astype(np.int32)
    g = _check_edges(rows[rowmap], lambda o: lap_solve_rows(rows, rowmap, return_info=True, opts=o))
    assert g["info"].gap_f64 > 0


def test_exact_through_the_row_map():
    from tools import instances
    rows = instances.typed_unique_cost(300, 1200, 11)[0]
    rowmap = np.repeat(np.arange(300), 4).astype(np.int32)
    g = lap_solve_rows(rows, rowmap, return_info=True, opts=dict(exact=1))
    c64 = rows[rowmap].astype(np.float64)
    opt = _opt(c64)
    assert g["info"].exact_status == 2
    assert abs(g["total"] - opt) <= 1e-12 * abs(opt) and abs(float(c64[np.arange(1200), g["rowsol"]].sum()) - opt) <= 1e-12 * abs(opt)
    assert np.array_equal(np.bincount(rowmap[g["colsol"]], minlength=300), np.full(300, 4))
    m = lap_solve(rows[rowmap], np.float32, return_info=True, opts=dict(exact=1))
    assert all(np.array_equal(g[k], m[k]) for k in ("rowsol", "colsol", "u", "v")) and g["total"] == m["total"]


def test_exact_batch_equals_single_problems():
    from tools import cross_unique, instances
    d = np.load(cross_unique.OUT)
    costs = [_i283()] + [cross_unique.instance(str(d["kind"][k]), int(d["n"][k]), int(d["seed"][k]), int(d["K"][k])) for k in (1, 2, 3)] + \
        [instances.typed_unique_cost(2003, 2003, 9)[0], np.random.default_rng(41).random((1500, 1500)).astype(np.float32)]
    bs = lap_solve_batch(costs, return_info=True, opts=dict(exact=1))
    for c, b in zip(costs, bs):
        s = lap_solve(c, np.float32, return_info=True, opts=dict(exact=1))
        assert all(np.array_equal(b[k], s[k]) for k in ("rowsol", "colsol", "u", "v")) and b["total"] == s["total"]
        assert b["info"].exact_status == s["info"].exact_status and b["info"].exact_edges == s["info"].exact_edges
    assert bs[0]["info"].exact_status == 2 and bs[0]["info"].exact_changed_rows > 0


def test_exact_overflow_pass_and_edge_cap():
    from tools import instances
    # rows with more near-tight columns than slots: emitted again, exactly; the same result as with the default 16 slots
    rows = instances.typed_unique_cost(300, 1200, 11)[0]
    c = rows[np.repeat(np.arange(300), 4)]
    for cc in (c, _additive(300)):
        a = lap_solve(cc, np.float32, return_info=True, opts=dict(exact=2))
        b = lap_solve(cc, np.float32, return_info=True, opts=dict(exact=1))
        assert a["info"].exact_status == 2 and a["info"].exact_overflow_rows > 0
        assert a["info"].exact_edges == b["info"].exact_edges
        assert all(np.array_equal(a[k], b[k]) for k in ("rowsol", "colsol", "u", "v")) and a["total"] == b["total"]
        opt = _opt(cc)
        assert abs(a["total"] - opt) <= 1e-12 * max(1.0, abs(opt))
    assert b["info"].exact_overflow_rows > 0                       # (additive: every row has hundreds)
    # over the cap (max(2^22, 32 n) edges): the float64 polish instead, the same result as polish = 1
    c = _additive(3000)
    g = lap_solve(c, np.float32, return_info=True, opts=dict(exact=1))
    p = lap_solve(c, np.float32, return_info=True, opts=dict(polish=1))
    assert g["info"].exact_status == 3 and g["info"].exact_edges > (1 << 22) and g["info"].polished == 1
    assert all(np.array_equal(g[k], p[k]) for k in ("rowsol", "colsol", "u", "v")) and g["total"] == p["total"]
    # ... in a batch too, one problem at a time after the batch
    bs = lap_solve_batch([c, _i283()], return_info=True, opts=dict(exact=1))
    assert bs[0]["info"].exact_status == 3 and np.array_equal(bs[0]["colsol"], p["colsol"]) and bs[1]["info"].exact_status == 2


def test_exact_is_a_no_op_when_the_certificate_is_zero():
    c = np.random.default_rng(5).integers(0, 10, (400, 400)).astype(np.float32)
    a = lap_solve(c, np.float32, return_info=True)
    g = lap_solve(c, np.float32, return_info=True, opts=dict(exact=1))
    assert g["info"].gap_f64 == 0.0 and g["info"].exact_status == 1 and g["info"].exact_edges == 0
    assert all(np.array_equal(a[k], g[k]) for k in ("rowsol", "colsol", "u", "v")) and a["total"] == g["total"]


def test_exact_argument_errors():
    c = np.random.default_rng(3).random((64, 64)).astype(np.float32)
    for bad in (dict(exact=-1), dict(exact=65), dict(exact=1, polish=1)):
        with pytest.raises(ValueError):
            lap_solve(c, np.float32, opts=bad)
    with pytest.raises(ValueError):
        lap_solve(c, np.float64, opts=dict(exact=1))
    with pytest.raises(ValueError):
        lapjv_hip(c, force_doubles=True, exact=True)
    L = _lib.lib()
    import ctypes
    o = _lib.LapOpts(exact=1)
    c64 = np.ascontiguousarray(c, np.float64)
    out = [np.empty(64, t) for t in (np.int32, np.int32, np.float64, np.float64)]
    st = L.cyto_lap_f64_opts(64, c64.ctypes.data, 64, 0, *[a.ctypes.data for a in out], None, None, 0, None, ctypes.byref(o))
    assert st == 1                                                 # CYTO_ERR_BAD_ARG
    assert lap_solve(c, np.float32, opts=dict(exact=64))["rowsol"].shape == (64,)


def test_exact_runs_are_bit_identical():
    c = _i283()
    a = lap_solve(c, np.float32, return_info=True, opts=dict(exact=1))
    b = lap_solve(c, np.float32, return_info=True, opts=dict(exact=1))
    assert all(np.array_equal(a[k], b[k]) for k in ("rowsol", "colsol", "u", "v")) and a["total"] == b["total"]
    assert a["info"].exact_edges == b["info"].exact_edges and a["info"].exact_changed_rows == b["info"].exact_changed_rows
