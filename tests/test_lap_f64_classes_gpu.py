"""The float64 LAP (lap_f64.hip, lap_chain.h) on every instance class, against the CPU restatements bit for bit: warm, cold, streaming.

The float64 solve sits behind lapjv_hip(force_doubles=True), lapjv_compat and cyto_lap_f64[_opts].  test_lap_gpu.py runs it on uniform
matrices, integer ties, one duplicated-row shape and one +-1e3 matrix; this file runs the classes of _f64_classes.py (few cell types --
what a CytoSPACE chunk is --, repeated rows, runs, the constant matrix, the c3 shape, negative values, and three classes whose costs
differ only below float32 resolution, the case force_doubles exists for) through the three ways a float64 solve can go:

    path      options                    restatement                             kernels
    warm      none (the default)         jv_oracle(c, float64, warm=True)        narrow, the float32 wide solve, widen_prices, then the chain
    cold      mode = 1                   jv_oracle(c, float64)                   jv_chain (n <= 4096), jv_chain_stream above
    stream1   chain_variant = 1          jv_oracle(c, float64)                   build_row_caches_wide + jv_chain_stream, colsol in LDS
    stream2   chain_variant = 2          jv_oracle(c, float64)                   jv_chain_stream without row caches
    stream3   chain_variant = 3          jv_oracle(c, float64)                   the caches, colsol in global memory (what n > 65 535 uses)

Every cell compares rowsol, colsol, u, v with np.array_equal, every key of STAT_KEYS, and the total within 1e-9 * max(1, |total|)
(test_lap_gpu.py: _check_warm).  Beside the restatement: colsol is a permutation with rowsol its inverse; the assignment's cost, summed
here from the float64 matrix, is scipy's optimum within 1e-9 * max(1, |opt|); on the classes with a generic unique optimum (UNIQUE) every
path returns scipy's indices element for element -- on sub32 the total proves nothing, the part of it that varies is ~1e-9 -- and on the
classes with repeated rows the spot of every column agrees between the warm and the cold result and scipy's (measured on the CPU
restatements: every one of those classes is unique at spot level at every size here, c3 included).

Sizes: 2, 5, 63, 64, 65, 300, 1200 for every class and path (8 for 2 and 5 where rows repeat, 10 for c3): WC_KC = 64 cache slots per row,
slot 63 the sentinel and floor, and build_row_caches_wide's n < WC_KC branch lie at 63 / 64 / 65.  4096 and 4100 (n <= 2 * VW * BLOCK = 4096
switches the register chain to the streaming chain) for warm and cold on sub32, dup4 and const, and warm alone on types at 4100 (the cold
oracle of types at 4100 takes 21 s).  The streaming variants are forced at the small sizes and need nothing above 1200.
One cut: types and types_pert run the cold and the streaming paths at n = 600 instead of 1200 (the warm path runs both).  Their cold
chain is cut at the row reduction's step budget, 2.2 million row scans in ONE workgroup whatever n is; on the first GPU run the cold
test of types at n = 1200 took 11.1 s and its streaming variants 10.5 / 14.9 / 15.8 s, oracle and scipy included.  What is left of that
cost: the budget-cut cells of the two classes take about 5 s each at n = 63, 65, 300, as do the three warm c3 cells named below.

That the intended path ran: info.f64_warm; the cold restatement of types hits the row reduction's step budget (arr_budget_hit) at every
n >= 65 and the warm one does not (it does at 63 too, not at 64); on sub32 the warm float64 phase does all the work (augmentations +
scans_arr > 0); with chain_variant = 1 at n = 1200 the row caches serve most scans on neg (hbm_row_reads < scans_redtransfer + scans_arr)
-- on types they mostly fail to certify, and the ratio is printed, not asserted.  Found on the way: the warm start of c3 at n = 63, 64, 65
hits the step budget too (a million row-reduction scans) while its cold solve does not.

scipy is the referee, and it is one only where its own float64 arithmetic is exact enough: on sub32 at n = 4100 its answer on the
float64 matrix is 3 units of 2^-52 ABOVE the optimum both restatements and the kernels return (five rows differ).  The indices of the
sub32 classes are therefore scipy's on the exact integer image of the matrix (_f64_classes.scipy_solve); the total is still compared
with scipy's on the float64 matrix.

Oracle and scipy time, measured on the finished pool in one process with 8 cores: 60 s -- 75 warm restatement solves 20 s, 72 cold
ones 10 s (the streaming cells share them), 75 instances through scipy 30 s (types at 4100 alone: 13 s).  Below the three-minute budget,
so no n = 4096 or 4100 cell was dropped.  345 class x path x size cells, 408 tests.  On an MI355X host the whole file takes 207 s, oracles and scipy included;
126 s of that are 21 budget-cut cells (4.7 ... 10 s each: types / types_pert cold and with chain_variant = 2 at n = 63, 65, 300, 600,
with chain_variant = 1 at 600, and warm c3 at 63, 64, 65); the four warm cells at n >= 4096 take 3.3 ... 3.8 s, every other test less
than 2 s.
"""
import numpy as np
import pytest

from cytospace_amd.lap import lap_solve
from oracle.jv import jv_oracle
from test_lap_gpu import STAT_KEYS
from _f64_classes import CLASSES, REPEATED, UNIQUE, make, scipy_solve, sizes, spots

pytestmark = pytest.mark.gpu

PATHS = {"warm": None, "cold": dict(mode=1), "stream1": dict(chain_variant=1), "stream2": dict(chain_variant=2),
         "stream3": dict(chain_variant=3)}
BUDGET_CUT = ("types", "types_pert")       # the cold chain runs into the row reduction's step budget: 2.2 million scans whatever n is
SMALL = [(cls, 600 if cls in BUDGET_CUT and n == 1200 else n) for cls in CLASSES for n in sizes(cls)]
BIG = [(cls, n) for n in (4096, 4100) for cls in ("sub32", "dup4", "const")]
WARM_CELLS = SMALL + [(cls, 1200) for cls in BUDGET_CUT] + BIG + [("types", 4100)]
COLD_CELLS = SMALL + BIG

# one matrix, one oracle solve per (instance, restatement), one checked GPU result per (instance, path)
_COSTS, _ORACLE, _GPU = {}, {}, {}


def _cost(cls, n):
    """(kept while it is small: the n >= 4096 ones are 134 MB each -- only the last one stays)"""
    if (cls, n) in _COSTS:
        return _COSTS[(cls, n)]
    c = make(cls, n)
    if n >= 4096:
        for k in [k for k in _COSTS if k[1] >= 4096]:
            del _COSTS[k]
    _COSTS[(cls, n)] = c
    return c


def _oracle(cls, n, warm):
    if (cls, n, warm) not in _ORACLE:
        _ORACLE[(cls, n, warm)] = jv_oracle(_cost(cls, n), np.float64, warm=warm)
    return _ORACLE[(cls, n, warm)]


def _solve(cls, n, path):
    """The GPU result of one cell, checked against its restatement and against scipy; solved once."""
    if (cls, n, path) in _GPU:
        return _GPU[(cls, n, path)]
    tag = (cls, n, path)
    c = _cost(cls, n)
    warm = path == "warm"
    o = _oracle(cls, n, warm)
    g = lap_solve(c, np.float64, return_info=True, opts=PATHS[path])
    info = g["info"]
    assert info.f64_warm == (1 if warm else 0), tag
    for k in ("rowsol", "colsol", "u", "v"):
        assert np.array_equal(g[k], o[k]), (tag, k)
    assert abs(g["total"] - o["total"]) <= 1e-9 * max(1.0, abs(o["total"])), (tag, g["total"], o["total"])
    gd, od = info.as_dict(), o["stats"].as_dict()
    for k in STAT_KEYS:
        assert gd[k] == od[k], (tag, k, gd[k], od[k])
    # not from the restatement: a permutation, and scipy's optimum of the float64 matrix
    ar = np.arange(n)
    assert np.array_equal(np.sort(g["colsol"]), ar) and np.array_equal(g["rowsol"][g["colsol"]], ar), tag
    sc_cols, opt = scipy_solve(cls, n, c)
    mine = float(c[ar, g["rowsol"]].sum())
    assert abs(mine - opt) <= 1e-9 * max(1.0, abs(opt)), (tag, mine, opt)
    if cls in UNIQUE:
        assert np.array_equal(g["rowsol"], sc_cols), tag
    # the intended path ran
    if cls == "types" and n >= 65:
        assert o["stats"].arr_budget_hit == (0 if warm else 1), tag
    if cls == "sub32" and warm and n >= 300:
        assert info.augmentations + info.scans_arr > 0, tag
    _GPU[(cls, n, path)] = g
    return g


def _id(cell):
    return f"{cell[0]}-{cell[1]}"


@pytest.mark.parametrize("cell", WARM_CELLS, ids=_id)
def test_warm(cell):
    _solve(*cell, "warm")


@pytest.mark.parametrize("cell", COLD_CELLS, ids=_id)
def test_cold(cell):
    _solve(*cell, "cold")


@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("cell", SMALL, ids=_id)
def test_stream(cell, variant):
    cls, n = cell
    g = _solve(cls, n, f"stream{variant}")
    if variant == 1 and (cls, n) in (("neg", 1200), ("types", 600)):
        i = g["info"]
        print(f"{cls} n={n} chain_variant=1: hbm_row_reads {i.hbm_row_reads} of {i.scans_redtransfer + i.scans_arr} "
              "reduction-transfer and row-reduction scans")
        if cls == "neg":
            assert i.hbm_row_reads < i.scans_redtransfer + i.scans_arr          # most scans were served by the caches


@pytest.mark.parametrize("cell", [c for c in COLD_CELLS if c[0] in REPEATED], ids=_id)
def test_spot_level_of_repeated_rows_is_one_answer(cell):
    # the slot inside a spot is the solver's choice, the spot is not: warm == cold == every streaming variant == scipy
    cls, n = cell
    loc = spots(cls, n)
    cold = loc[_solve(cls, n, "cold")["colsol"]]
    assert np.array_equal(loc[_solve(cls, n, "warm")["colsol"]], cold)
    if cell in SMALL:
        for v in (1, 2, 3):
            assert np.array_equal(loc[_solve(cls, n, f"stream{v}")["colsol"]], cold), v
    sc_cols, _ = scipy_solve(cls, n)
    assert np.array_equal(loc[np.argsort(sc_cols)], cold)


@pytest.mark.parametrize("cell", [c for c in WARM_CELLS if c[0] in UNIQUE and c in COLD_CELLS], ids=_id)
def test_unique_classes_have_one_answer_on_every_path(cell):
    # (each path equals scipy's indices in _solve already; this states the claim between the paths themselves)
    cls, n = cell
    paths = ["warm", "cold"] + (["stream1", "stream2", "stream3"] if cell in SMALL else [])
    first = _solve(cls, n, paths[0])
    for p in paths[1:]:
        g = _solve(cls, n, p)
        assert np.array_equal(g["rowsol"], first["rowsol"]) and np.array_equal(g["colsol"], first["colsol"]), p
