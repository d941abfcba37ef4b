"""float64 references of the cost build's intermediate results and the checks that compare a float32 device result with them.

TEST INFRASTRUCTURE ONLY -- never imported by cytospace_amd/.  Every reference here is the obvious formula, not the device's
formulation: two-pass mean and standard deviation, pandas.DataFrame.rank() for the ranks, explicit differences for the
Euclidean distance.  Used by tests/test_cost_precision_gpu.py; the checks themselves are pinned on the CPU by
tests/test_precision_helpers_cpu.py.
"""
import numpy as np

from . import cost as ocost

STANDARDIZE, RANK, RAW = 0, 1, 2          # CYTO_TRANSFORM_* (include/cytohip.h)


def normalized(x, already_normalized):
    """The values the transform sees: np.nan_to_num(x) when already normalised, else normalize_data (common.py:142-147)."""
    x = np.asarray(x).astype(np.float64)
    return np.nan_to_num(x) if already_normalized else ocost.normalize_data(x)


def ranks(v):
    """pandas.DataFrame(v).rank(): per column, ascending, ties averaged, 1-based (matrix_correlation_spearman)."""
    import pandas as pd
    return pd.DataFrame(np.asarray(v, dtype=np.float64)).rank().to_numpy()


def operand(x, transform, already_normalized):
    """The GEMM operand of one matrix in float64.  Returns (r64, delta):
    r64   the standardised values (STANDARDIZE), the standardised average-tie ranks (RANK) or the values themselves (RAW);
          columns of zero variance hold the reference's division by zero (NaN / inf);
    delta per entry, the float64 error of y - mean next to the column mean, 1e-12 (|y| + |mean|) / (std sqrt(G)): where z is
          tiny its float32 spacing is below that noise.  0 for RAW."""
    y = normalized(x, already_normalized)
    if transform == RANK:
        y = ranks(y)
    if transform == RAW:
        return y, np.zeros_like(y)
    G = y.shape[0]
    mean = y.mean(axis=0)
    d = y - mean
    std = np.sqrt((d * d).mean(axis=0))                    # population std (ddof = 0), two passes
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (std * np.sqrt(G))
        r = d * inv
        delta = 1e-12 * (np.abs(y) + np.abs(mean)) * inv
    return r, delta


def ulp_report(z, r64, delta):
    """Compare a float32 result z with its float64 reference entry by entry (finite entries of r64 only).
    Returns a dict:
      excess      max over entries of |z - r64| - spacing(float32(r64)) - delta (<= 0: every entry within one float32 ulp)
      differ      entries where z != float32(r64)
      unexplained entries where z != float32(r64) and r64 is neither within 1e-10 relative of a float32 rounding midpoint nor
                  within delta of z (a correctly rounded float64 result cannot land there)
      where       (row, col) of the worst entry"""
    z = np.asarray(z, dtype=np.float32)
    r64 = np.asarray(r64, dtype=np.float64)
    fin = np.isfinite(r64)
    r = np.where(fin, r64, 0.0)
    d = np.where(fin, delta, 0.0)
    r32 = r.astype(np.float32)
    zf = np.where(fin, z, r32).astype(np.float64)
    sp = np.spacing(np.abs(r32)).astype(np.float64)
    err = np.abs(zf - r) - sp - d
    differ = (zf != r32.astype(np.float64)) & fin
    # the float32 neighbour of float32(r64) on r64's side, and the midpoint between the two
    toward = np.where(r32.astype(np.float64) > r, np.float32(-np.inf), np.float32(np.inf))
    nb = np.nextafter(r32, toward.astype(np.float32)).astype(np.float64)
    mid = 0.5 * (r32.astype(np.float64) + nb)
    near_mid = np.abs(r - mid) <= 1e-10 * np.abs(r)
    unexplained = differ & ~near_mid & ~(np.abs(zf - r) <= d)
    k = int(np.argmax(err)) if err.size else 0
    return dict(excess=float(err.max()) if err.size else -1.0, differ=int(differ.sum()), unexplained=int(unexplained.sum()),
                where=np.unravel_index(k, err.shape) if err.size else None)


def euclidean(st, sc):
    """Spots x cells Euclidean distances, sqrt(sum_g (a_g - b_g)^2) over explicit differences in float64 (scipy's cdist loop,
    what linear_assignment_solvers.py:58-59 calls)."""
    from scipy.spatial.distance import cdist
    return cdist(np.asarray(st, dtype=np.float64).T, np.asarray(sc, dtype=np.float64).T, "euclidean")


def cost(metric, sc, st, already_normalized=False):
    """The float64 cost of calculate_cost's lapjv branch without the row repeats, spots x cells: -Pearson, -Spearman or the
    Euclidean distance of the normalised matrices."""
    a, b = normalized(sc, already_normalized), normalized(st, already_normalized)
    if metric == "Pearson_correlation":
        return -ocost.matrix_correlation_pearson(a, b)
    if metric == "Spearman_correlation":
        return -ocost.matrix_correlation_pearson(ranks(a), ranks(b))
    if metric == "Euclidean":
        return euclidean(b, a)
    raise ValueError(metric)


def cost_error(metric, got, ref):
    """The contract's error measure: absolute for the correlations (2e-6, README), relative for Euclidean (2e-6)."""
    e = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if metric == "Euclidean":
        e = e / np.maximum(ref, 1e-30)
    return e


def dual_lower_bound(ref_rows, rowmap, u, v):
    """A lower bound on the optimum of the LAP whose row i is ref_rows[rowmap[i]] (float64), from ANY duals u, v:
    sum(u) + sum(v) - n * max(0, max violation of ref - u - v >= 0).  Independent of how u, v were obtained."""
    ref_rows = np.asarray(ref_rows, dtype=np.float64)
    rowmap = np.asarray(rowmap)
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    umax = np.full(ref_rows.shape[0], -np.inf)
    np.maximum.at(umax, rowmap, u)
    used = np.isfinite(umax)
    worst = ((ref_rows[used] - v[None, :]).min(axis=1) - umax[used]).min()
    n = len(rowmap)
    return float(u.sum() + v.sum() - n * max(0.0, -worst))
