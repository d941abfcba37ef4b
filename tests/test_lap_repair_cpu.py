"""CPU tests (no GPU) of cyto_lap_repair_sparse, the host half of cyto_lap_opts.exact: successive shortest paths over a sparse edge
set E that contains the starting permutation, against scipy's exact solver on the same sparse problem (missing edges infinite)."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from cytospace_amd.lap import lap_repair_sparse


def _csr(n, edges):
    """edges: per row a list of (col, r) -> row_ptr, cols, r"""
    row_ptr = np.zeros(n + 1, np.int64)
    cols, rs = [], []
    for i in range(n):
        row_ptr[i + 1] = row_ptr[i] + len(edges[i])
        for j, r in edges[i]:
            cols.append(j)
            rs.append(r)
    return row_ptr, np.array(cols, np.int32), np.array(rs, np.float64)


def _dense(n, edges):
    d = np.full((n, n), np.inf)
    for i in range(n):
        for j, r in edges[i]:
            d[i, j] = min(d[i, j], r)
    return d


def _instance(rng, n, kind):
    """A starting permutation pi with r_i,pi(i) = 0 and extra edges: `real` (continuous r, some negative), `ties` (small integers:
    many equal distances), `sparse` (most rows hold only their own edge)"""
    pi = rng.permutation(n).astype(np.int32)
    p = {"real": min(1.0, 4.0 / n), "ties": min(1.0, 6.0 / n), "sparse": min(1.0, 0.5 / n)}[kind]
    edges = []
    for i in range(n):
        e = [(int(pi[i]), 0.0)]
        for j in np.flatnonzero(rng.random(n) < p):
            if j == pi[i]:
                continue
            if kind == "ties":
                r = float(rng.integers(-2, 3))
            else:
                r = float(rng.normal()) * (1e-7 if rng.random() < 0.5 else 1.0)
            e.append((int(j), r))
        order = rng.permutation(len(e))                      # (the starting edge need not come first)
        edges.append([e[k] for k in order])
    return pi, edges


def _check(pi, edges):
    n = len(pi)
    row_ptr, cols, r = _csr(n, edges)
    got = lap_repair_sparse(pi, row_ptr, cols, r)
    assert np.array_equal(np.sort(got), np.arange(n))
    d = _dense(n, edges)
    assert np.all(np.isfinite(d[np.arange(n), got])), "an edge outside E"
    rr, cc = linear_sum_assignment(d)
    opt = float(d[rr, cc].sum())
    mine = float(d[np.arange(n), got].sum())
    assert abs(mine - opt) <= 1e-12 * max(1.0, np.abs(d[np.isfinite(d)]).sum()), (mine, opt)
    return got, d


@pytest.mark.parametrize("kind", ["real", "ties", "sparse"])
def test_repair_matches_scipy_on_random_sparse_instances(kind):
    rng = np.random.default_rng({"real": 11, "ties": 12, "sparse": 13}[kind])
    for _ in range(100):
        n = int(rng.integers(5, 401)) if rng.random() < 0.3 else int(rng.integers(5, 60))
        pi, edges = _instance(rng, n, kind)
        got, d = _check(pi, edges)
        # rows that hold only their own edge can go nowhere else
        for i in range(n):
            if len(edges[i]) == 1:
                assert got[i] == pi[i]
        if kind == "ties":                                   # (integer costs: the optimum's total exactly)
            rr, cc = linear_sum_assignment(d)
            assert d[np.arange(n), got].sum() == d[rr, cc].sum()


def test_rows_that_cannot_improve_keep_their_column():
    # two blocks without edges between them: the first has rows with a cheaper edge than their own (freed), the second none -- its
    # rows sit on a minimum of their row (ties at r = 0 included) and no augmenting path reaches them: every one keeps its column
    rng = np.random.default_rng(21)
    for _ in range(40):
        a, b = int(rng.integers(3, 80)), int(rng.integers(3, 80))
        n = a + b
        pa, pb = rng.permutation(a), a + rng.permutation(b)
        pi = np.concatenate([pa, pb]).astype(np.int32)
        edges = []
        for i in range(n):
            e = [(int(pi[i]), 0.0)]
            lo, hi = (0, a) if i < a else (a, n)
            for j in range(lo, hi):
                if j != pi[i] and rng.random() < 0.15:
                    r = float(rng.integers(-3, 4)) if i < a else float(rng.integers(0, 3))
                    e.append((j, r))
            edges.append(e)
        got, _ = _check(pi, edges)
        assert np.array_equal(got[a:], pi[a:])


def test_repair_is_deterministic_and_leaves_an_optimal_start_alone():
    rng = np.random.default_rng(31)
    pi, edges = _instance(rng, 300, "ties")
    row_ptr, cols, r = _csr(300, edges)
    a = lap_repair_sparse(pi, row_ptr, cols, r)
    assert np.array_equal(a, lap_repair_sparse(pi, row_ptr, cols, r))
    # every r >= 0: nothing is freed, nothing moves
    r0 = np.abs(r)
    assert np.array_equal(lap_repair_sparse(pi, row_ptr, cols, r0), pi)


def test_repair_argument_errors():
    pi = np.array([1, 0, 2], np.int32)
    row_ptr, cols, r = _csr(3, [[(1, 0.0)], [(0, 0.0)], [(2, 0.0)]])
    assert np.array_equal(lap_repair_sparse(pi, row_ptr, cols, r), pi)
    with pytest.raises(ValueError):                          # not a permutation
        lap_repair_sparse(np.array([1, 1, 2], np.int32), row_ptr, cols, r)
    with pytest.raises(ValueError):                          # row 0's own edge is missing
        lap_repair_sparse(np.array([2, 0, 1], np.int32), row_ptr, cols, r)
    with pytest.raises(ValueError):                          # column out of range
        lap_repair_sparse(pi, row_ptr, np.array([1, 0, 3], np.int32), r)
    with pytest.raises(ValueError):                          # non-finite cost
        lap_repair_sparse(pi, row_ptr, cols, np.array([0.0, np.nan, 0.0]))


def test_exact_option_argument_errors_need_no_device():
    # cyto_lap_opts.exact is validated before any device is touched: out of 0 ... 64, with polish, or on a float64 entry point
    from cytospace_amd import _lib
    from cytospace_amd.lap import lap_solve, lapjv_hip
    import ctypes
    assert ctypes.sizeof(_lib.LapOpts) == 20 * 4                 # (exact took one of the reserved words: the struct keeps its size)
    c = np.random.default_rng(3).random((16, 16)).astype(np.float32)
    for dtype, bad in ((np.float32, dict(exact=-1)), (np.float32, dict(exact=65)), (np.float32, dict(exact=1, polish=1)),
                       (np.float64, dict(exact=1))):
        with pytest.raises(ValueError):
            lap_solve(c, dtype, opts=bad)
    with pytest.raises(ValueError):
        lapjv_hip(c, force_doubles=True, exact=True)
    assert _lib.LapInfo().exact_status == 0


def test_polish_on_a_batch_is_refused_without_a_device():
    # cyto_lap_opts.polish belongs to the single-problem calls: cyto_lap_batch_f32_opts refuses it for the whole call, every
    # problem's status included, before a device is selected (a batch used to return unpolished results with polished == 0)
    from cytospace_amd.lap import lap_solve_batch
    costs = [np.random.default_rng(s).random((16, 16)).astype(np.float32) for s in (1, 2, 3)]
    for opts in (dict(polish=1), dict(polish=1, certify=1), dict(polish=1, mode=1)):
        with pytest.raises(ValueError, match="status 1:"):
            lap_solve_batch(costs, opts=opts)
        with pytest.raises(ValueError, match="status 1:"):
            lap_solve_batch(costs, opts=opts, return_status=True)

