"""oracle/precision.py: the references and checks tests/test_cost_precision_gpu.py holds the device's cost build to, pinned on the
CPU.  A float32 operand computed by the device's formulation (one-pass moments in float64, one rounding at the end) must pass the
one-ulp check; the same operand with one entry off by one float32 ulp, or a mean off by 1e-9, must not."""
import numpy as np

from oracle import cost as ocost
from oracle import precision as P


def _device_formulation(x):
    # what transform_write_v / col_finish_moments compute: sums of y and y^2 in float64, var = E[y^2] - mean^2, one rounding
    y = ocost.normalize_data(x.astype(np.float64))
    G = y.shape[0]
    m = y.sum(0) / G
    var = np.maximum((y * y).sum(0) / G - m * m, 0.0)
    inv = 1.0 / (np.sqrt(var) * np.sqrt(G))
    return ((y - m) * inv).astype(np.float32)


def test_device_formulation_passes_and_one_ulp_more_fails():
    rng = np.random.default_rng(0)
    x = rng.poisson(rng.lognormal(0, 1.5, (20000, 1)) * 0.3, (20000, 6)).astype(np.float64)
    r64, delta = P.operand(x, P.STANDARDIZE, 0)
    z = _device_formulation(x)
    rep = P.ulp_report(z, r64, delta)
    assert rep["excess"] <= 0 and rep["unexplained"] == 0, rep
    bad = z.copy()
    i = np.argmax(np.abs(r64[:, 2]))
    bad[i, 2] = np.nextafter(bad[i, 2], np.float32(np.inf) if bad[i, 2] >= r64[i, 2] else np.float32(-np.inf))   # away from r64
    assert P.ulp_report(bad, r64, delta)["unexplained"] == 1
    y = ocost.normalize_data(x)
    off = ((y - (y.mean(0) + 1e-9)) / (y.std(0) * np.sqrt(y.shape[0]))).astype(np.float32)
    assert P.ulp_report(off, r64, delta)["unexplained"] > 0


def test_ranks_are_pandas_average_ties_and_signed_zeros_tie():
    rng = np.random.default_rng(1)
    v = rng.choice(np.array([-0.0, 0.0, 1.5, -2.25]), (500, 3))
    r = P.ranks(v)
    assert np.array_equal(r, ocost.rank_columns(v))
    zeros = v == 0
    for c in range(3):
        assert len(np.unique(r[zeros[:, c], c])) == 1


def test_zero_variance_columns_are_non_finite_in_the_reference():
    x = np.zeros((40, 3))
    x[:, 1] = np.arange(40)
    x[:, 2] = 2.0
    r, _ = P.operand(x, P.STANDARDIZE, 1)
    assert not np.isfinite(r[:, 0]).any() and np.isfinite(r[:, 1]).all() and not np.isfinite(r[:, 2]).any()
    r, _ = P.operand(x, P.RANK, 1)
    assert not np.isfinite(r[:, 0]).any() and np.isfinite(r[:, 1]).all()


def test_euclidean_reference_is_explicit_differences():
    rng = np.random.default_rng(2)
    a, b = rng.random((50, 4)), rng.random((50, 7))
    d = P.euclidean(a, b)
    assert d.shape == (4, 7)
    assert np.allclose(d, np.sqrt(((a.T[:, None, :] - b.T[None, :, :]) ** 2).sum(-1)), rtol=1e-15, atol=0)


def test_dual_lower_bound_is_the_optimum_for_optimal_duals_and_below_it_otherwise():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(3)
    rows = rng.random((6, 18))
    rowmap = np.repeat(np.arange(6), 3)
    full = rows[rowmap]
    r, c = linear_sum_assignment(full)
    best = full[r, c].sum()
    u = full.min(axis=1)                                     # feasible, not optimal
    assert P.dual_lower_bound(rows, rowmap, u, np.zeros(18)) <= best + 1e-12
    assert P.dual_lower_bound(rows, rowmap, u + 0.5, np.zeros(18)) <= best + 1e-12     # infeasible duals: the bound still holds
