# The cost build (cytospace_amd/csrc/cost.hip) against float64 references at production shapes: the GEMM operand of all three
# transforms to one float32 ulp, the contraction of all three metrics to the documented tolerances, and what the remaining error
# means for the assignment.  References: oracle/precision.py (two-pass moments, pandas ranks, explicit-difference distances).
import ctypes

import numpy as np
import pytest

from cytospace_amd import _lib
from cytospace_amd import common as gcommon
from cytospace_amd import cytospace as gcyto
from cytospace_amd.lap import lap_solve, lap_solve_rows
from oracle import precision as P
from tools import instances

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (np.float32, 0), "f64": (np.float64, 1), "u16": (np.uint16, 2), "u8": (np.uint8, 3)}
TRANSFORMS = {"standardize": P.STANDARDIZE, "rank": P.RANK, "raw": P.RAW}
METRIC_ID = gcommon.METRICS
TOL = 2e-6        # Pearson / Spearman: absolute (README); Euclidean: relative


def _up(x, m):
    return -(-x // m) * m


# ---- 1. the GEMM operand (cyto_transform) ----------------------------------------------------------------------------------

def _transform(x, transform, already, on_device):
    """cyto_transform into a z buffer pre-filled with 0xFF bytes (NaN).  Host input: ld = C (the 4-column kernels when C % 4 == 0).
    Device input: a pitch ldx % 4 != 0 and a 1-element pointer offset (the 1-column kernels), every element of the buffer that is not
    data poisoned (NaN; the integer types: their maximum): nothing of it may reach a column sum, a moment or a rank.  Returns the
    whole Gpad x ldz buffer."""
    L = _lib.lib()
    G, C = x.shape
    Gpad, ldz = _up(G, 32), _up(C, 128)
    z = _lib.DeviceBuffer.from_numpy(np.full(Gpad * ldz * 4, 0xFF, np.uint8))
    dt = [v[1] for v in DTYPES.values() if v[0] == x.dtype.type][0]
    try:
        if not on_device:
            _lib.check(L.cyto_transform(transform, G, C, x.ctypes.data, C, dt, 0, already, z.ptr, ldz, Gpad, 0, None))
        else:
            ldx = C + 1 if (C + 1) % 4 else C + 2
            host = np.full(G * ldx + 1, np.nan if x.dtype.kind == "f" else np.iinfo(x.dtype).max, x.dtype)
            host[1:].reshape(G, ldx)[:, :C] = x
            xd = _lib.DeviceBuffer.from_numpy(host)
            try:
                _lib.check(L.cyto_transform(transform, G, C, xd.ptr + x.itemsize, ldx, dt, 1, already, z.ptr, ldz, Gpad, 0, None))
            finally:
                xd.free()
        return z.to_numpy((Gpad, ldz), np.float32)
    finally:
        z.free()


def _value_classes(G, C, dtype, transform, already, rng):
    """Counts of a few magnitudes plus the columns where kernels go wrong (as many of them as C leaves room for; the last column
    stays an ordinary one)."""
    is_float = dtype in (np.float32, np.float64)
    hi = 255 if dtype == np.uint8 else 65535
    lam = rng.lognormal(0.0, 1.5, G)[:, None] * rng.lognormal(0.0, 0.5, C)[None, :]
    x = np.minimum(rng.poisson(lam), hi).astype(np.float64)
    if G >= 2:                                           # (no column is constant by accident)
        x[np.arange(C) % G, np.arange(C)] = 0
        x[(np.arange(C) + 1) % G, np.arange(C)] = 1 + np.arange(C) % 7
    classes = ["zero", "single", "large"]
    if is_float:
        classes.append("tiny")
    if is_float and not already and transform != P.RANK:
        classes += ["negative_nan", "pos_inf", "neg_inf"]    # (the log2_cleaned path; ranks are taken of the cleaned input)
    if is_float and already:
        classes.append("signed_zero_ties")
    if already:
        classes.append("constant")
    for c, kind in enumerate(classes[:max(0, C - 1)]):
        col = np.zeros(G)
        if kind == "single":
            col[rng.integers(G)] = rng.integers(1, hi + 1)
        elif kind == "large":
            col = rng.integers(0, hi + 1, G).astype(np.float64)
            col[rng.random(G) < 0.3] = 0
            col[rng.integers(G)] = hi
        elif kind == "tiny":                                 # fractional values, column sum far below 1: t up to 1e6 in log2_ge1
            col = rng.random(G) * (1e-30 if dtype == np.float32 else 1e-100 if already else 1e-300)
        elif kind == "negative_nan":                         # t < 0 and 0 < t < 1 next to ordinary counts; NaN -> 0
            col = x[:, c].copy()
            k = rng.permutation(G)
            col[k[:max(1, G // 8)]] = -0.5 - rng.random(max(1, G // 8)) * 3
            if G >= 2:
                col[k[-1]] = np.nan
        elif kind in ("pos_inf", "neg_inf"):                 # +-inf -> +-max finite, the column sum with it
            col = x[:, c] + rng.random(G)
            col[rng.integers(G)] = np.inf if kind == "pos_inf" else -np.inf
        elif kind == "signed_zero_ties":                     # d2ord's + 0.0: -0.0 and +0.0 are one tie
            col = rng.choice(np.array([-0.0, 0.0, 1.5, -2.25]), G, p=[0.35, 0.35, 0.2, 0.1])
        elif kind == "constant":
            col[:] = 2.0
        x[:, c] = col
    return x.astype(dtype)


SMALL_G = (1, 31, 32, 33, 255, 256, 257)
ALL_C = (1, 3, 4, 5, 255, 256, 257, 1027)
OPERAND_SHAPES = [(G, C) for G in SMALL_G for C in ALL_C] + [(4100, 4), (4100, 5), (4100, 257), (20000, 4), (20000, 5), (20000, 256)]
RANK_EXTRA_SHAPES = [(36601, 4), (36601, 5)]       # two rank_columns launches, the MOWN = 32 variant


@pytest.mark.parametrize("already", [0, 1])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_transform_operand_within_one_ulp_of_float64(transform, dtype, already):
    tr, dt = TRANSFORMS[transform], DTYPES[dtype][0]
    shapes = OPERAND_SHAPES + (RANK_EXTRA_SHAPES if tr == P.RANK else [])
    rng = np.random.default_rng(1000 * tr + 10 * DTYPES[dtype][1] + already)
    failures, differ, entries = [], 0, 0
    for G, C in shapes:
        x = _value_classes(G, C, dt, tr, already, rng)
        r64, delta = P.operand(x, tr, already)
        assert np.isfinite(P.normalized(x, already)).all()          # (the data avoid log2(0) = -inf by construction)
        zh = _transform(x, tr, already, on_device=False)
        zd = _transform(x, tr, already, on_device=True)
        Gpad, ldz = zh.shape
        tag = f"G={G} C={C}"
        # layout equivalence: the 4-column and 1-column kernels give the same bits (standardize_dev's claim)
        if not np.array_equal(zh.view(np.uint32), zd.view(np.uint32)):
            failures.append(f"{tag}: host (ld = C) and device (pitch {C + 1 if (C + 1) % 4 else C + 2}, offset 1) inputs differ "
                            f"in {(zh.view(np.uint32) != zd.view(np.uint32)).sum()} words")
        # the padding contract: +0.0 in rows G..Gpad and columns C..ldz, nothing left of the 0xFF fill in the G x C block
        pad = np.concatenate([zh[G:].ravel(), zh[:G, C:].ravel()]).view(np.uint32)
        if (pad != 0).any():
            failures.append(f"{tag}: {(pad != 0).sum()} padding words are not +0.0")
        z = zh[:G, :C]
        # zero-variance columns: non-finite exactly where the reference divides by zero
        ref_bad = ~np.isfinite(r64).all(axis=0)
        got_bad = ~np.isfinite(z)
        if not np.array_equal(got_bad.any(axis=0), ref_bad) or not got_bad[:, ref_bad].all():
            failures.append(f"{tag}: non-finite columns {np.flatnonzero(got_bad.any(axis=0))[:8]}, "
                            f"reference divides by zero in {np.flatnonzero(ref_bad)[:8]}")
        if tr == P.RAW and np.isnan(z).any():
            failures.append(f"{tag}: NaN in the RAW operand")
        rep = P.ulp_report(z, r64, delta)
        differ += rep["differ"]
        entries += int(np.isfinite(r64).sum())
        if rep["excess"] > 0 or rep["unexplained"]:
            i, j = rep["where"]
            failures.append(f"{tag}: worst entry ({i}, {j}) z={z[i, j]!r} ref={r64[i, j]!r} exceeds one ulp + delta by "
                            f"{rep['excess']:.3g}; {rep['unexplained']} entries differ from float32(ref) without a near-midpoint "
                            f"reference")
    print(f"\n[operand] {transform} {dtype} already={already}: {differ} of {entries} finite entries differ from float32(ref), "
          f"all near a rounding midpoint or within delta")
    assert not failures, "\n".join(failures[:12])


# ---- 2. the contraction (cyto_cost_metric) -----------------------------------------------------------------------------------

SENTINEL = np.float32(-12345.25)


def _counts(G, n, rng, depth):
    lam = depth * rng.lognormal(0.0, 1.5, G)[:, None] * rng.lognormal(0.0, 0.5, (1, n))
    x = rng.poisson(lam).astype(np.float32)
    x[rng.integers(G, size=n), np.arange(n)] += 1            # (no all-zero column: zero variance is section 1's case)
    x[rng.integers(G, size=n), np.arange(n)] += 2
    return x


def _cost_metric(metric, zst, zsc, slots, rows, ldc):
    """cyto_cost_metric into a rows x ldc buffer pre-filled with SENTINEL; returns the whole buffer."""
    buf = _lib.DeviceBuffer.from_numpy(np.full((rows, ldc), SENTINEL, np.float32))
    try:
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        ms = ctypes.c_double()
        _lib.check(_lib.lib().cyto_cost_metric(METRIC_ID[metric], zst.Gpad, zst.C, zsc.C, zst.buf.ptr, zst.ld, zsc.buf.ptr, zsc.ld,
                                               slots.ctypes.data, buf.ptr, ldc, ctypes.byref(ms), 0, None))
        return buf.to_numpy((rows, ldc), np.float32)
    finally:
        buf.free()


def _sample_rows(S, rng):
    """Every tile row's first and last spot and one more: each 128 x 128 output tile is visited by the comparison."""
    rows = set()
    for m0 in range(0, S, 128):
        last = min(S, m0 + 128) - 1
        rows.update({m0, last, int(rng.integers(m0, last + 1))})
    return np.array(sorted(rows))


METRICS = ["Pearson_correlation", "Spearman_correlation", "Euclidean"]
TILE_SHAPES = {                         # (S, C) -> tiles_m x tiles_n
    "one_tile": (100, 120),
    "8x8": (1024, 1024),
    "9x9": (1100, 1100),
    "17x10": (2100, 1250),
    "1x65": (60, 8200),
    "65x1": (8200, 70),
    "S,C=1_mod_128": (129, 385),
}


@pytest.mark.parametrize("G", [32, 97, 2000])
@pytest.mark.parametrize("metric", METRICS)
def test_contraction_against_float64_over_the_tile_walk(metric, G):
    rng = np.random.default_rng(G)
    failures, report = [], []
    for name, (S, C) in TILE_SHAPES.items():
        sc, st = _counts(G, C, rng, 0.3), _counts(G, S, rng, 3.0)
        zsc = gcommon.StandardizedMatrix(sc, False, 0, metric)
        zst = gcommon.StandardizedMatrix(st, False, 0, metric)
        ldc = _up(C, 4)
        got = _cost_metric(metric, zst, zsc, np.ones(S), S, ldc)
        zsc.buf.free()
        zst.buf.free()
        if (got[:, :C] == SENTINEL).any() or not np.isfinite(got[:, :C]).all():
            failures.append(f"{name}: {(got[:, :C] == SENTINEL).sum()} entries not written, "
                            f"{(~np.isfinite(got[:, :C])).sum()} non-finite")
            continue
        rows = _sample_rows(S, rng) if S > 256 else np.arange(S)
        ref = P.cost(metric, sc, st[:, rows])
        err = P.cost_error(metric, got[rows, :C], ref)
        report.append(f"{name} S={S} C={C}: {err.max():.3g}")
        if err.max() > TOL:
            i, j = np.unravel_index(np.argmax(err), err.shape)
            failures.append(f"{name} S={S} C={C}: max error {err.max():.3g} at spot {rows[i]} cell {j} "
                            f"(got {got[rows[i], j]!r}, ref {ref[i, j]!r})")
    print(f"\n[contraction] {metric} G={G} max error: " + "; ".join(report))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("G,C,S", [(20000, 4096, 512), (36601, 2048, 256)])
@pytest.mark.parametrize("metric", METRICS)
def test_contraction_against_float64_at_full_gene_counts(metric, G, C, S):
    # full 10x gene sets (c3: 20 000; unfiltered: 36 601), ~8 cells per spot: 64 spot rows against all cells on the host
    sc, st, _ = instances.synth_expression(G, C, S, seed=G % 97)
    zsc = gcommon.StandardizedMatrix(sc, False, 0, metric)
    zst = gcommon.StandardizedMatrix(st, False, 0, metric)
    ldc = _up(C, 4)
    got = _cost_metric(metric, zst, zsc, np.ones(S), S, ldc)
    zsc.buf.free()
    zst.buf.free()
    rows = np.sort(np.random.default_rng(0).choice(S, 64, replace=False))
    ref = P.cost(metric, sc, st[:, rows])
    err = P.cost_error(metric, got[rows, :C], ref)
    i, j = np.unravel_index(np.argmax(err), err.shape)
    msg = (f"{metric} G={G} S={S} C={C}: max {'relative' if metric == 'Euclidean' else 'absolute'} error {err.max():.3g} "
           f"(mean {err.mean():.3g}) at spot {rows[i]} cell {j}: got {got[rows[i], j]!r}, ref {ref[i, j]!r}")
    print("\n[full genes] " + msg)
    assert err.max() <= TOL, msg


@pytest.mark.parametrize("metric", METRICS)
def test_rowstart_epilogue_repeats_zero_slots_and_stays_in_bounds(metric):
    # slots with repeats and zeros across the tile edges: every LAP row is its spot's row of the identity build, bit for bit; the
    # padding columns (ldc > C) and one extra row keep the sentinel
    rng = np.random.default_rng(5)
    G, S, C = 97, 300, 260
    sc, st = _counts(G, C, rng, 0.3), _counts(G, S, rng, 3.0)
    slots = rng.integers(0, 4, S)
    slots[[0, 127, 128, 255, 256, S - 1]] = [0, 3, 0, 0, 2, 0]
    N = int(slots.sum())
    zsc = gcommon.StandardizedMatrix(sc, False, 0, metric)
    zst = gcommon.StandardizedMatrix(st, False, 0, metric)
    ldc = _up(C, 4) + 12
    ident = _cost_metric(metric, zst, zsc, np.ones(S), S + 1, ldc)
    rep = _cost_metric(metric, zst, zsc, slots, N + 1, ldc)
    zsc.buf.free()
    zst.buf.free()
    for name, buf, n in (("identity", ident, S), ("repeats", rep, N)):
        assert (buf[:n, C:] == SENTINEL).all(), f"{name}: a store beyond column C"
        assert (buf[n] == SENTINEL).all(), f"{name}: a store beyond the last row"
    loc = np.repeat(np.arange(S), slots)
    assert np.array_equal(rep[:N, :C].view(np.uint32), ident[loc, :C].view(np.uint32))
    ref = P.cost(metric, sc, st)
    err = P.cost_error(metric, ident[:S, :C], ref)
    assert err.max() <= TOL, f"{metric}: max error {err.max():.3g}"


# ---- 3. what the error means for the assignment -----------------------------------------------------------------------------

def _eps(metric, ref):
    return TOL * (float(np.abs(ref).max()) if metric == "Euclidean" else 1.0)


@pytest.mark.parametrize("metric", ["Spearman_correlation", "Euclidean"])
def test_split_path_duals_certify_the_float64_cost(metric):
    # a chunk-sized instance: the device cost (pearson_cost_device) solved by the device LAP; its duals must be feasible and
    # complementary on the float64 reference cost to within the cost build's tolerance
    G, C, S = 3000, 3000, 300
    sc, st, slots = instances.synth_expression(G, C, S, seed=31)
    cost, N, ld, _ = gcommon.pearson_cost_device(sc, st, slots, already_normalized=False, metric=metric)
    try:
        g = lap_solve(None, np.float32, device_ptr=cost.ptr, n=N, ld=ld)
    finally:
        cost.free()
    ref = P.cost(metric, sc, st)
    eps = _eps(metric, ref)
    loc = np.repeat(np.arange(S), slots)
    red = ref[loc] - g["u"].astype(np.float64)[:, None] - g["v"].astype(np.float64)[None, :]
    slack = np.abs(red[np.arange(N), g["rowsol"]])
    msg = f"{metric}: min reduced cost {red.min():.3g}, max slack {slack.max():.3g}, 2 eps = {2 * eps:.3g}"
    print("\n[duals] " + msg)
    assert red.min() >= -2 * eps, msg
    assert slack.max() <= 2 * eps, msg


def _lsap_optimum(ref, slots):
    from scipy.optimize import linear_sum_assignment
    full = ref[np.repeat(np.arange(len(slots)), slots)]
    r, c = linear_sum_assignment(full)
    return float(full[r, c].sum())


@pytest.mark.parametrize("metric", ["Spearman_correlation", "Euclidean"])
def test_fused_and_context_totals_on_the_float64_cost(metric):
    G, C, S = 2000, 2400, 240
    sc, st, slots = instances.synth_expression(G, C, S, seed=32)
    ref = P.cost(metric, sc, st)
    eps = _eps(metric, ref)
    mapped = gcyto.assign_pearson(sc, st, slots, already_normalized=False, distance_metric=metric)
    assert np.array_equal(np.bincount(mapped, minlength=S), slots)
    mine, best = float(ref[mapped, np.arange(C)].sum()), _lsap_optimum(ref, slots)
    assert best - 1e-9 * abs(best) <= mine <= best + 2 * C * eps, (metric, "fused", mine, best)
    # a chunk of the context path: half the cells against every spot, per-chunk slot counts
    rng = np.random.default_rng(3)
    slot_of = rng.permutation(np.repeat(np.arange(S), slots))
    idx = np.sort(rng.permutation(C)[:C // 2])
    sub = np.bincount(slot_of[idx], minlength=S)
    with gcyto.ExpressionContext(sc, st, False, 0, metric) as ctx:
        m2 = ctx.assign_chunk(idx, sub)
    assert np.array_equal(np.bincount(m2, minlength=S), sub)
    mine2, best2 = float(ref[m2, idx].sum()), _lsap_optimum(ref[:, idx], sub)
    print(f"\n[totals] {metric}: fused {mine - best:.3g} above the optimum, context chunk {mine2 - best2:.3g} "
          f"(bound 2 n eps = {2 * C * eps:.3g}, {C * eps:.3g})")
    assert best2 - 1e-9 * abs(best2) <= mine2 <= best2 + 2 * len(idx) * eps, (metric, "context", mine2, best2)


def test_spearman_block_pipeline_total_on_the_float64_cost():
    # C > 16 384 takes the fused path's block pipeline (cells uploaded, ranked and contracted in blocks of 8 192, the first a quarter)
    G, C, S = 240, 17200, 1720
    sc, st, slots = instances.synth_expression(G, C, S, seed=33)
    mapped = gcyto.assign_pearson(sc, st, slots, already_normalized=False, distance_metric="Spearman_correlation")
    assert np.array_equal(np.bincount(mapped, minlength=S), slots)
    ref = P.cost("Spearman_correlation", sc, st)
    mine = float(ref[mapped, np.arange(C)].sum())
    # the optimum of the float64 cost from below: any duals certify a lower bound (here the device solver's on the rounded
    # reference: n = 17 000 is beyond a host assignment solver in this file's time budget)
    loc = np.repeat(np.arange(S), slots)
    g = lap_solve_rows(ref.astype(np.float32), loc)
    lb = P.dual_lower_bound(ref, loc, g["u"], g["v"])
    print(f"\n[block pipeline] Spearman: {mine - lb:.3g} above the dual bound (2 n eps = {2 * C * TOL:.3g})")
    assert lb - 1e-6 <= mine <= lb + 2 * C * TOL, (mine, lb)
