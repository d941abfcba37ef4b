"""The float64 instance classes of test_lap_f64_classes_gpu.py and test_oracle_cpu.py: seeded, numpy only, made in float64 (nothing is
cast up from float32 except the c3 shape, which tools.instances builds in float32), every value within a few binades of 1 or 1e3.

    types      few cell types (kind 2 of test_lap_batch_gpu.py, in float64): what a CytoSPACE chunk looks like.  The cold classic chain
               hits the row reduction's step budget on it, the warm start does not
    types_pert types + 1e-16 * rng.random
    dup4       every row four times (kind 3)
    runs       long runs of one row (kind 4)
    const      np.full((n, n), 3.0) (kind 6)
    c3         tools.instances.c3_shaped_cost cut to n x n (kind 7), widened, plus CytoSPACE's 1e-16 * rand (cytospace.py:325-327)
    neg        -1e3 * rng.random
    sub32      1 + 1e-9 * rng.random: the narrowed copy is ONE float32 value, the warm prices carry no information
    sub32few   1 + 4e-7 * rng.random: the narrowed copy has a handful of values, heavy float32 ties over a float64-unique optimum
    sub32dup   every row of a 1 + 1e-10 * rng.random base four times

make(cls, n) -> the matrix; spots(cls, n) -> the spot (distinct row) of every row for the classes with repeated rows, else None;
scipy_solve(cls, n) -> linear_sum_assignment on the float64 matrix, once per instance.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

CLASSES = ("types", "types_pert", "dup4", "runs", "const", "c3", "neg", "sub32", "sub32few", "sub32dup")
UNIQUE = ("types", "types_pert", "neg", "sub32", "sub32few")     # a generic, unique optimum: every exact solver returns the same indices
REPEATED = ("dup4", "runs", "sub32dup", "c3")                    # repeated rows: unique at spot level at most
BASE_SIZES = (2, 5, 63, 64, 65, 300, 1200)
_SEED = {c: k for k, c in enumerate(CLASSES)}
_SCIPY = {}


def sizes(cls, base=BASE_SIZES):
    """The sizes of `base` a class exists at: four copies of a row / runs of a row need n >= 8, ten slots per spot n >= 10 -- those
    classes take n = 8 (n = 10) instead of 2 and 5."""
    lo = 10 if cls == "c3" else 8 if cls in REPEATED else 0
    out = []
    for n in base:
        n = max(n, lo)
        if n not in out:
            out.append(n)
    return out


def _types(rng, n):
    prof = rng.normal(size=(5, 48))
    rows = prof[rng.integers(0, 5, n)] + 0.05 * rng.normal(size=(n, 48))
    cols = prof[rng.integers(0, 5, n)] + 0.05 * rng.normal(size=(n, 48))
    return -(rows @ cols.T)


def _run_len(n):
    m = n // 100 or 1
    return (n + m - 1) // m


def make(cls, n):
    rng = np.random.default_rng([_SEED[cls], n])
    if cls == "types":
        c = _types(rng, n)
    elif cls == "types_pert":
        c = _types(np.random.default_rng([_SEED["types"], n]), n) + 1e-16 * rng.random((n, n))
    elif cls == "dup4":
        c = np.repeat(rng.random(((n + 3) // 4, n)), 4, axis=0)[:n]
    elif cls == "runs":
        c = np.repeat(-(rng.random((n // 100 or 1, n)) ** 3), _run_len(n), axis=0)[:n]
    elif cls == "const":
        c = np.full((n, n), 3.0)
    elif cls == "c3":
        from tools import instances
        c32, _ = instances.c3_shaped_cost((n + 9) // 10 * 10, 10, 3)
        c = c32[:n, :n].astype(np.float64) + 1e-16 * np.random.RandomState(1).rand(n, n)
    elif cls == "neg":
        c = -1e3 * rng.random((n, n))
    elif cls == "sub32":
        c = 1.0 + 1e-9 * rng.random((n, n))
    elif cls == "sub32few":
        c = 1.0 + 4e-7 * rng.random((n, n))
    elif cls == "sub32dup":
        c = np.repeat(1.0 + 1e-10 * rng.random(((n + 3) // 4, n)), 4, axis=0)[:n]
    else:
        raise ValueError(cls)
    c = np.ascontiguousarray(c)
    assert c.dtype == np.float64 and c.shape == (n, n)
    return c


def spots(cls, n):
    if cls in ("dup4", "sub32dup"):
        return np.arange(n) // 4
    if cls == "runs":
        return np.arange(n) // _run_len(n)
    if cls == "c3":
        return np.arange(n) // 10
    return None


def exact_image(cls, c):
    """The sub32 classes as integers: c = 1 + k * 2^-52 with k < 2^40, so k = (c - 1) * 2^52 is exact in float64, has the same optimal
    assignments as c, and every sum and difference a solver forms on it is exact.  None for the other classes."""
    if not cls.startswith("sub32"):
        return None
    k = (c - 1.0) * 2.0 ** 52
    assert np.array_equal(k, np.rint(k)) and k.min() >= 0 and k.max() < 2.0 ** 40 and np.array_equal(1.0 + k * 2.0 ** -52, c)
    return k


def scipy_solve(cls, n, c=None):
    """(scipy's column of every row, scipy's total of the float64 matrix), summed as the tests sum theirs.

    The total is linear_sum_assignment's on the float64 matrix, always.  So are the indices, except on the sub32 classes: there scipy's
    own float64 duals round (values near 1 that differ from the 31st bit on), and at n = 4100 its answer on the float64 matrix is NOT
    the optimum -- 3 units of 2^-52 above it, five rows different (measured; both restatements and scipy on the integer image agree
    on the better assignment).  The indices of those classes come from scipy on exact_image, where its arithmetic is exact: the same
    solver on the same problem, and the true optimum.  At every other size of those classes the two scipy solves return the same
    indices (n = 2 ... 1200 and 4096, measured)."""
    if (cls, n) not in _SCIPY:
        c = make(cls, n) if c is None else c
        r, cc = linear_sum_assignment(c)
        assert np.array_equal(r, np.arange(n))
        opt = float(c[r, cc].sum())
        k = exact_image(cls, c)
        if k is not None:
            r, cc = linear_sum_assignment(k)
            assert np.array_equal(r, np.arange(n))
        _SCIPY[(cls, n)] = (cc, opt)
    return _SCIPY[(cls, n)]
