"""The reference of test_lap_ranges_*_gpu.py, pinned where it runs without a GPU: the CPU restatements (oracle/jv.py) on the pool of
_ranges.py -- costs scaled by 2^+-40 and 2^+-100, below the normal range, with -0.0, with hundreds of binades in one matrix -- and the
float64 restatements, cold and warm, at 2^+-100, 2^-140 and 2^+-900.

The GPU tests compare the kernels with the oracle of the scaled matrix bit for bit.  That is worth what the oracle is worth there, so
here, for every instance and both float32 restatements (jv_oracle: the chain solver's, jv_oracle_wide: the wide solver's):

  1. the gate: a permutation, finite duals, max(|u|, |v|) < 2^126.  No instance whose intermediates could overflow reaches a kernel;
  2. exact zone (c * 2^k, the image exact): the base solve's indices, its duals times 2^k bit for bit, every counter equal -- except
     the wide restatement's gap_exp, the exponent FIELD of the median gap, which is the base's + k where the base's is not 0 (0 is
     the field of a zero gap -- integer ties, repeated rows -- and a zero gap stays zero at every scale) --, total = base total * 2^k;
  3. negzero: everything equal to the kind-5 base (-0.0 == 0.0 as a cost);
  4. optimality against scipy.optimize.linear_sum_assignment on the float64 image, without an invented tolerance: with
     viol_i = max(0, (c - v)[i, rowsol_i] - min_j (c - v)[i, j]) in float64 from the oracle's own duals (the certificate of
     test_lap_gpu.py::test_float64_certificate_of_a_float32_solve), -1e-12 * sum|c_assigned| <= mine - opt <= sum viol; and
     mine == opt on subgrid, sub126, sub130, binades_pos and every kind-1 / kind-5 instance of the exact zone;
  5. float64: jv_oracle(c * 2^k, float64, warm) on the classes types, neg, dup4, sub32few of _f64_classes.py, n = 65 and 300.  Cold at
     every k, and warm at k = +-100: the base solve's indices and exactly scaled duals.  Warm at k = -900, -140, 900 (the narrowed image
     is zero, subnormal and inexact, or infinite: the warm start carries nothing or something else): a permutation whose total is
     scipy's on the scaled matrix within 1e-12 relative.

The 136 float32 instances (the pool's 127 and the n = 96 group of the batch test) and the 80 float64 cells take 34 s on 8 cores, scipy
included; the slowest solves are the wide restatement of few cell types at n = 2100, 3.7 s each.
"""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import _f64_classes
import _ranges
from oracle.jv import jv_oracle

NAMES = _ranges.names()
GATED = NAMES + [nm for nm in _ranges.batch_group(96) + ["kind5-96"] if nm not in NAMES]     # (the batch test's n = 96 group and its base)
_SCIPY = {}


def _scipy_opt(nm):
    if nm not in _SCIPY:
        c64 = _ranges.cost(nm).astype(np.float64)
        r, cc = linear_sum_assignment(c64)
        assert np.array_equal(r, np.arange(len(c64)))
        _SCIPY[nm] = float(c64[r, cc].sum())
    return _SCIPY[nm]


def test_the_pool_is_what_the_gpu_tests_expect():
    assert len(NAMES) == len(set(NAMES)) == 127
    assert all(_ranges.name(*_ranges.parts(nm)) == nm for nm in NAMES)
    at_2100 = [nm for nm in NAMES if _ranges.parts(nm)[1] == 2100]
    assert sorted(at_2100) == sorted([_ranges.name(kd, 2100, k) for kd in (1, 2) for k in (-100, 0, 100)] + ["subgrid-2100"])
    assert [nm for nm in NAMES if nm.startswith("top")] == ["top-65"]
    assert all(nm in GATED for n in (96, 300) for nm in _ranges.batch_group(n)) and len(GATED) == 127 + 9
    assert [nm for nm in NAMES if _ranges.parts(nm)[2] and not _ranges.is_exact_zone(nm)] == list(_ranges.INEXACT)
    for nm in ("sub126-300", "sub130-300", "subgrid-300"):
        c = _ranges.cost(nm)
        assert 0 < np.abs(c).max() < 2.0 ** -125 and (np.abs(c[c != 0]) < 2.0 ** -126).any()       # subnormal values
    c = _ranges.cost("sub130-300").astype(np.float64) * 2.0 ** 130
    assert not np.array_equal(c, _ranges.base(1, 300))                                               # an inexact image
    for nm, lo, hi in (("binades_pos-300", 190, 200), ("binades_signed-300", 110, 120)):
        e = np.log2(np.abs(_ranges.cost(nm).astype(np.float64)))
        assert lo < e.max() - e.min() <= hi


@pytest.mark.parametrize("chain", [False, True], ids=["wide", "chain"])
@pytest.mark.parametrize("nm", GATED)
def test_oracle_across_the_float_range(nm, chain):
    what, n, k = _ranges.parts(nm)
    c = _ranges.cost(nm)
    o = _ranges.oracle(nm, chain)
    ar = np.arange(n)
    # 1. the gate
    assert np.array_equal(np.sort(o["colsol"]), ar) and np.array_equal(o["rowsol"][o["colsol"]], ar)
    assert np.isfinite(o["u"]).all() and np.isfinite(o["v"]).all()
    assert max(np.abs(o["u"]).max(), np.abs(o["v"]).max()) < 2.0 ** 126
    # 2. / 3. the base solve, scaled
    bn = _ranges.base_of(nm)
    if bn is not None:
        b = _ranges.oracle(bn, chain)
        s = 2.0 ** k
        assert np.array_equal(o["rowsol"], b["rowsol"]) and np.array_equal(o["colsol"], b["colsol"])
        for key in ("u", "v"):
            assert np.array_equal(o[key].astype(np.float64), b[key].astype(np.float64) * s), key
            if what != "negzero":                                   # (there u = c - v takes the sign of a zero cost)
                assert np.array_equal(np.signbit(o[key]), np.signbit(b[key])), key
        od, bd = o["stats"].as_dict(), b["stats"].as_dict()
        if "gap_exp" in bd and bd["gap_exp"] > 0:
            bd["gap_exp"] += k
        assert od == bd
        assert abs(o["total"] - b["total"] * s) <= 1e-12 * abs(b["total"] * s)
    # 4. scipy on the float64 image
    c64 = c.astype(np.float64)
    opt = _scipy_opt(nm)
    mine = float(c64[ar, o["rowsol"]].sum())
    red = c64 - o["v"].astype(np.float64)[None, :]
    viol = np.maximum(red[ar, o["rowsol"]] - red.min(1), 0.0)
    assert -1e-12 * float(np.abs(c64[ar, o["rowsol"]]).sum()) <= mine - opt <= float(viol.sum()), (mine, opt, float(viol.sum()))
    if what in ("subgrid", "sub126", "sub130", "binades_pos", "top", 1, 5):
        assert mine == opt, (mine, opt)


# ---- 5. the float64 restatements ----

F64_CLASSES = ("types", "neg", "dup4", "sub32few")
_F64 = {}


def _f64(cls, n, k, warm):
    if (cls, n, k, warm) not in _F64:
        _F64[(cls, n, k, warm)] = jv_oracle(_f64_classes.make(cls, n) * 2.0 ** k, np.float64, warm=warm)
    return _F64[(cls, n, k, warm)]


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("k", [-900, -140, -100, 100, 900])
@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("cls", F64_CLASSES)
def test_float64_oracle_across_the_double_range(cls, n, k, warm):
    c = _f64_classes.make(cls, n)
    s = 2.0 ** k
    cs = c * s
    assert np.isfinite(cs).all() and np.array_equal(cs / s, c)                      # exact in float64
    o = _f64(cls, n, k, warm)
    ar = np.arange(n)
    assert np.array_equal(np.sort(o["colsol"]), ar) and np.array_equal(o["rowsol"][o["colsol"]], ar)
    assert np.isfinite(o["u"]).all() and np.isfinite(o["v"]).all()
    with np.errstate(over="ignore"):
        narrowed = cs.astype(np.float32)
    if abs(k) == 100:
        assert np.isfinite(narrowed).all() and (narrowed != 0).any()
    elif k == 900:
        assert np.isinf(narrowed).all()
    elif k == -900:
        assert not narrowed.any()
    else:
        assert (np.abs(narrowed) < 2.0 ** -126).all() and narrowed.any()            # subnormal images
    if not warm or abs(k) == 100:
        b = _f64(cls, n, 0, warm)
        assert np.array_equal(o["rowsol"], b["rowsol"]) and np.array_equal(o["colsol"], b["colsol"])
        assert np.array_equal(o["u"], b["u"] * s) and np.array_equal(o["v"], b["v"] * s)
        assert o["stats"].as_dict() == b["stats"].as_dict()
    else:
        r, cc = linear_sum_assignment(cs)
        opt = float(cs[r, cc].sum())
        assert abs(float(cs[ar, o["rowsol"]].sum()) - opt) <= 1e-12 * abs(opt)
        assert abs(o["total"] - opt) <= 1e-12 * abs(opt)
