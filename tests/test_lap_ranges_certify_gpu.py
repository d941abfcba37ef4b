"""The float64 certificate, the exact repair and the polish of a float32 solve, under power-of-two scaling.

The instance is the near tie of test_lap_gpu.py::test_polish_recovers_the_unique_optimum_on_a_near_tie (instance 283 of
tests/golden/cross_unique.npz: few cell types, n = 2 973): the default float32 solve ends above the optimum, its certificate is positive,
and the repair / the polish move rows.  It is solved at c * 2^k, k = -100, -40, 0, 40, 100 -- the image is exact (asserted by
_ranges.scaled) --, as a single problem and through a row map that stores every row once; the exact option also as ONE batch holding
the five scales.

Scaling by 2^k commutes with every operation of the float32 solve, with the float64 differences and sums of the certificate and with
tau = gap * (1 + 2^-30).  So, at every k:

  certify = 1   gap_rows is k = 0's; gap_f64 and gap_max_f64 are k = 0's times 2^k EXACTLY; and both are numpy's on the scaled matrix
                (test_lap_gpu.py::test_float64_certificate_of_a_float32_solve's expression: gap_max exactly, gap_f64 within 1e-12
                relative -- relative to the gap itself: that test's 1e-12 * max(1, gap) is an absolute bound that means nothing at 2^-100)
  exact = 1, 2  exact_status, exact_edges, exact_free_rows, exact_changed_rows, exact_overflow_rows and rowsol are k = 0's; rowsol is
                scipy's on the float64 image (the optimum is unique); v is the certify = 1 solve's bit for bit
  polish = 1    polished == 1; rowsol is k = 0's and scipy's

8 s for the file on an MI355X host; scipy (once per scale, 1.3 s) is most of it.
"""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import _ranges
from cytospace_amd.lap import lap_solve, lap_solve_batch, lap_solve_rows

pytestmark = pytest.mark.gpu

SCALES = (-100, -40, 0, 40, 100)
HOW = ("single", "rowmap")
EXACT_KEYS = ("exact_status", "exact_edges", "exact_free_rows", "exact_changed_rows", "exact_overflow_rows")
_COST, _SCIPY, _GPU = {}, {}, {}


def _cost(k):
    if k not in _COST:
        if k == 0:
            from tools import cross_unique
            _COST[0] = np.ascontiguousarray(cross_unique.instance("typed", 2973, 5283, 4))
        else:
            _COST[k] = _ranges.scaled(_cost(0), k)
    return _COST[k]


def _scipy(k):
    if k not in _SCIPY:
        r, cc = linear_sum_assignment(_cost(k).astype(np.float64))
        assert np.array_equal(r, np.arange(len(cc)))
        _SCIPY[k] = cc
    return _SCIPY[k]


def _solve(k, how, **opts):
    key = (k, how, tuple(sorted(opts.items())))
    if key not in _GPU:
        c = _cost(k)
        if how == "rowmap":
            g = lap_solve_rows(c, np.arange(len(c), dtype=np.int32), return_info=True, opts=opts)
        else:
            g = lap_solve(c, np.float32, return_info=True, opts=opts)
        _GPU[key] = g
    return _GPU[key]


def _viol(c, g):
    n = len(c)
    red = c.astype(np.float64) - g["v"].astype(np.float64)[None, :]
    return np.maximum(red[np.arange(n), g["rowsol"]] - red.min(1), 0.0)


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("k", SCALES)
def test_certificate_scales_exactly(k, how):
    i0 = _solve(0, how, certify=1)["info"]
    assert i0.certified == 1 and i0.gap_f64 > 0 and i0.gap_rows > 0            # the instance is a near tie: there is a gap to scale
    g = _solve(k, how, certify=1)
    i = g["info"]
    assert i.certified == 1 and i.gap_rows == i0.gap_rows
    assert i.gap_f64 == i0.gap_f64 * 2.0 ** k and i.gap_max_f64 == i0.gap_max_f64 * 2.0 ** k
    viol = _viol(_cost(k), g)
    assert i.gap_rows == int((viol > 0).sum()) and i.gap_max_f64 == viol.max()
    assert abs(i.gap_f64 - viol.sum()) <= 1e-12 * viol.sum()
    b = _solve(0, how, certify=1)
    assert np.array_equal(g["rowsol"], b["rowsol"]) and np.array_equal(g["v"].astype(np.float64), b["v"].astype(np.float64) * 2.0 ** k)


def _check_exact(g, k, how, exact):
    tag = (k, how, exact)
    i, i0 = g["info"], _solve(0, how, exact=exact)["info"]
    assert i0.exact_status == 2 and i0.exact_changed_rows > 0 and i0.exact_edges > 0, tag
    for key in EXACT_KEYS:
        assert getattr(i, key) == getattr(i0, key), (tag, key, getattr(i, key), getattr(i0, key))
    assert np.array_equal(g["rowsol"], _solve(0, how, exact=exact)["rowsol"]), tag
    assert np.array_equal(g["rowsol"], _scipy(k)), tag
    assert np.array_equal(g["v"], _solve(k, how, certify=1)["v"]), tag


@pytest.mark.parametrize("exact", [1, 2])
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("k", SCALES)
def test_exact_repair_is_the_same_at_every_scale(k, how, exact):
    _check_exact(_solve(k, how, exact=exact), k, how, exact)


@pytest.mark.parametrize("exact", [1, 2])
def test_exact_repair_in_one_batch_of_five_scales(exact):
    res = lap_solve_batch([_cost(k) for k in SCALES], return_info=True, opts=dict(exact=exact))
    assert len(res) == len(SCALES)
    for k, g in zip(SCALES, res):
        _check_exact(g, k, "single", exact)                         # (k = 0's are the single solve's: a batch changes nothing)


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("k", SCALES)
def test_polish_is_the_same_at_every_scale(k, how):
    g = _solve(k, how, polish=1)
    assert g["info"].polished == 1
    assert np.array_equal(g["rowsol"], _solve(0, how, polish=1)["rowsol"])
    assert np.array_equal(g["rowsol"], _scipy(k))
