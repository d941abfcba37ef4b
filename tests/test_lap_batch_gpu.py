"""Batched LAP solves against the CPU oracle, bit for bit: same-size groups, sub-batches, slices, failures, device costs.

A batch (cyto_lap_batch_f32_opts -> lap_batch_any -> lap_batch_same_n -> lap_solve_f32_batch -> wide_solve_batch / chain_solve_batch)
is what a CytoSPACE run executes: the chunks of a rank have ONE size, so a production batch is one large same-size group.  The claim
(cytohip.h): a problem's indices, duals and semantic counters are the oracle's bit for bit, whatever shares its launches.
Nothing here has a tolerance except `total`, a float64 sum compared within BASELINE.json's 1e-5 * max(1, |total|).

The reference is the CPU oracle alone (jv_oracle_wide for the default / mode=2, jv_oracle for mode=1), solved ONCE per distinct
instance (the cache below is keyed by the instance's name; groups repeat instances on purpose).  A single GPU solve is never the
reference; (f) and (g) use device results only where no CPU value exists (the context's own cost rows, the float64 certificate).

Group sizes and the constant of the driver each one is there for:
  n (a):  1, 2, 3, 5      want_groups = n >= 2, `if (n >= 2 && !resume)`: the degenerate launches (lap_jv.hip, lap_wide_rr.hip)
          63, 64, 65      KC = 63 cached columns per row / one wave: the row cache holds the whole row, exactly, or misses one column
          300, 1000       the plain LDS-resident sizes (jv_chain2<2 / 5, true>)
          2100, 4200      the n >= 2048 and n >= 4096 rules of wide_solve_batch (whole-chip first rounds, long-list rounds in wide_arr)
  nb (b): 2, 5            below every threshold
          9               straddles 2048 / min(nb, 8), the grid of wide_rt (wide_launch_rt), with 5 below it
          16, 17          straddle 2048 / min(nb, 16), the grid of wide_sc_init / wide_sc_wipe (wide_launch_arr) -- and 16 is the
                          first group dealt over G = 2 sub-batches (batch.hip: cnt >= 16), so a LAUNCH sees 16 or 17 problems only in
                          the larger groups below
          33              G = 4 sub-batches (cnt >= 32) of 9 / 8 / 8 / 8; 4096 / nb and 1024 / nb (wide_launch_claims) do not divide evenly
          130             G = 8 sub-batches (cnt >= 128), seg_quorum = nl / 4 = 4 (n = 96 only)
          15, 68, 127     what ONE launch carries: a sub-batch holds nb / G problems, so the lists above put at most 9 (n = 1000) or 17
                          (n = 96) problems into a launch.  15 is the largest group that is not dealt out, 68 gives four launches of
                          17 (at n = 1000 the first count where bid_total / nb = 240 is below the n / 4 = 250 workgroups a round would
                          take), 127 four of 32 / 32 / 32 / 31 -- the most one launch carries without a developer knob (256 / 8), which
                          is why bid_total / nb never reaches its floor of 64 here
  (c):    11 problems sliced by max_concurrent 1, 2, 3, 4 (`lo += conc` in lap_batch_any_impl runs 11, 6, 4, 3 times), 0 = one slice
  (d):    6 and 17 problems with rejected ones among them (the SolveJob list shorter than the job list; 17: inside a sub-batch)
  (i):    cyto_lap_opts.polish, which a batch does not have: refused for the call, and the next batch is the oracle's

Oracle time, measured on the finished pool in one process with 8 cores: 60 s for the 597 oracle solves of (a)-(e), (g), (h) --
(a) 38 s, of which the group at n = 4200 takes 30 s; (b) 12 s; (g) 9 s; the rest 2 s.  (f)'s 40 chunk oracles work on cost rows that
come from the device and are not in that figure: each of its four tests takes less than a second on a GPU host, oracles included.
Below the 5-minute budget, so nothing was cut: all eight kinds
run at n = 4200.
"""
import threading

import numpy as np
import pytest

from cytospace_amd import _lib
from cytospace_amd.lap import lap_solve, lap_solve_batch, lap_solve_batch_device
from oracle.jv import jv_oracle, jv_oracle_wide
from test_lap_gpu import STAT_KEYS, WIDE_KEYS

pytestmark = pytest.mark.gpu

WIDE, CHAIN = dict(mode=2), dict(mode=1)
NONFINITE = _lib.CYTO_ERR_NONFINITE
KINDS = (1, 2, 3, 4, 5, 6, 7, 8)
NEED_8_ROWS = (3, 4, 7)        # four copies of a row, runs of a row, ten slots per spot: no such matrix below n = 8


# ---- the instance pool: seeded, numpy only, nothing read from disk ----

_COSTS, _ORACLE = {}, {}


def _make(kind, n, seed):
    rng = np.random.default_rng([kind, n, seed])
    if kind == 1:        # uniform: the eps-scaled phases
        return rng.random((n, n)).astype(np.float32)
    if kind == 2:        # few cell types: scales, asks for cache rebuilds, deep searches
        prof = rng.normal(size=(5, 48)).astype(np.float32)
        rows = prof[rng.integers(0, 5, n)] + 0.05 * rng.normal(size=(n, 48)).astype(np.float32)
        cols = prof[rng.integers(0, 5, n)] + 0.05 * rng.normal(size=(n, 48)).astype(np.float32)
        return -(rows @ cols.T).astype(np.float32)
    if kind == 3:        # every row four times: never scales, same_prev set, wide_claim_*
        return np.repeat(rng.random(((n + 3) // 4, n)), 4, axis=0)[:n].astype(np.float32)
    if kind == 4:        # long runs of one row
        m = n // 100 or 1
        return np.repeat(-(rng.random((m, n)) ** 3), (n + m - 1) // m, axis=0)[:n].astype(np.float32)
    if kind == 5:        # integer ties
        return rng.integers(0, 10, (n, n)).astype(np.float32)
    if kind == 6:        # a constant matrix: every distance equal, the plateau case
        return np.full((n, n), 3.0, np.float32)
    if kind == 7:        # the c3 shape (every search one edge), cut to n x n
        from tools import instances
        c, _ = instances.c3_shaped_cost((n + 9) // 10 * 10, 10, 3 + seed)
        return np.ascontiguousarray(c[:n, :n])
    if kind == 8:        # kind 1 scaled by 1e3, sign flipped: negative and large values
        return (-1e3 * rng.random((n, n))).astype(np.float32)
    raise ValueError(kind)


def _name(kind, n, seed=0):
    return f"k{kind}_n{n}_s{seed}"


def _cost(name):
    """The matrix of an instance name (kept while it is small: the n = 4200 ones are rebuilt, 70 MB each)."""
    if name in _COSTS:
        return _COSTS[name]
    kind, n, seed = (int(x[1:]) for x in name.split("_"))
    c = _make(kind, n, seed)
    if n <= 2100:
        _COSTS[name] = c
    return c


def _oracle(name, chain, rounds=0, cost=None):
    key = (name, bool(chain), rounds)
    if key not in _ORACLE:
        c = _cost(name) if cost is None else cost
        _ORACLE[key] = jv_oracle(c, np.float32) if chain else jv_oracle_wide(c, np.float32, max_rounds=-1 if rounds == 0 else rounds)
    return _ORACLE[key]


def _kinds_at(n):
    return [k for k in KINDS if n >= 8 or k not in NEED_8_ROWS]


def _equals_oracle(g, name, chain, rounds=0, tag="", cost=None):
    """One problem of a batch against its oracle: indices and duals bit for bit, every semantic counter, the total, info.wide."""
    o = _oracle(name, chain, rounds, cost)
    for k in ("rowsol", "colsol", "u", "v"):
        assert np.array_equal(g[k], o[k]), (tag, name, k)
    assert abs(g["total"] - o["total"]) <= 1e-5 * max(1.0, abs(o["total"])), (tag, name, g["total"], o["total"])     # BASELINE.json
    gd, od = g["info"].as_dict(), o["stats"].as_dict()
    assert gd["wide"] == (0 if chain else 1), (tag, name)
    if chain:
        for k in STAT_KEYS:
            assert gd[k] == od[k], (tag, name, k, gd[k], od[k])
    else:
        for kg, ko in WIDE_KEYS:
            assert gd[kg] == od[ko], (tag, name, kg, gd[kg], od[ko])


def _solve_and_check(names, opts, chain, tag="", **kw):
    res = lap_solve_batch([_cost(nm) for nm in names], return_info=True, opts=opts, **kw)
    assert len(res) == len(names)
    for b, (nm, g) in enumerate(zip(names, res)):
        _equals_oracle(g, nm, chain, tag=f"{tag} problem {b} of {len(names)}")
    return res


def _bits(res):
    return [tuple(r[k].tobytes() for k in ("rowsol", "colsol", "u", "v")) + (r["total"],) for r in res]


# ---- (a) same-size groups, both solvers ----

@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 300, 1000, 2100, 4200])
def test_a_one_group_of_every_kind(n):
    # ONE group of all kinds that exist at n (kinds 3, 4, 7 need n >= 8: NEED_8_ROWS, so the groups at n = 1, 2, 3, 5 hold five
    # problems), as one call: the wide solver by name, the chain solver, and what a caller gets without options (the wide solver)
    names = [_name(k, n) for k in _kinds_at(n)]
    assert len(names) == (8 if n >= 8 else 5)
    if n == 4200:
        costs = [_make(k, n, 0) for k in _kinds_at(n)]          # (built once for the three calls, dropped with the test)
        for nm, c in zip(names, costs):
            _oracle(nm, False, cost=c), _oracle(nm, True, cost=c)
    else:
        costs = [_cost(nm) for nm in names]
    for opts, chain in ((WIDE, False), (CHAIN, True), (None, False)):
        res = lap_solve_batch(costs, return_info=True, opts=opts)
        assert len(res) == len(names)
        for b, (nm, g) in enumerate(zip(names, res)):
            _equals_oracle(g, nm, chain, tag=f"opts={opts} problem {b}")


# ---- (b) the number of problems ----

_GROUPS = {}


def _distinct_group(n, nb):
    """nb problems of size n whose oracle results differ pairwise (so a result in a neighbour's slot is a mismatch, not a
    coincidence): the kinds in turn, every visit of a seeded kind with a seed of its own, kinds 6 and 7 once.  A candidate whose
    colsol -- of either oracle -- equals that of a problem already in the group is dropped for the next seed; three seeds in a row
    without a new problem retire a kind (at n = 96 that is kind 4: ONE row 96 times, which reduces to the constant matrix of
    kind 6 whatever the seed; at n = 1000 its ten rows give every seed an answer of its own)."""
    if (n, nb) in _GROUPS:
        return _GROUPS[(n, nb)]
    names, seen = [], {False: set(), True: set()}
    seed = {k: 0 for k in KINDS}
    retired = set()
    while len(names) < nb:
        progressed = False
        for k in (1, 2, 3, 6, 7, 4, 5, 8):                      # (kind 6 ahead of kind 4: see above)
            if len(names) == nb:
                break
            if k in retired:
                continue
            for _ in range(1 if k in (6, 7) else 3):
                nm = _name(k, n, seed[k])
                seed[k] += 1
                cs = {ch: _oracle(nm, ch)["colsol"].tobytes() for ch in (False, True)}
                if all(cs[ch] not in seen[ch] for ch in (False, True)):
                    names.append(nm)
                    for ch in (False, True):
                        seen[ch].add(cs[ch])
                    progressed = True
                    break
            else:
                retired.add(k)
            if k in (6, 7):
                retired.add(k)
        assert progressed, "the pool cannot supply another distinct problem"
    _GROUPS[(n, nb)] = names
    return names


@pytest.mark.parametrize("chain", [False, True], ids=["wide", "chain"])
@pytest.mark.parametrize("n,nb", [(96, 2), (96, 5), (96, 9), (96, 16), (96, 17), (96, 33), (96, 130),
                                  (1000, 2), (1000, 5), (1000, 9), (1000, 16), (1000, 17), (1000, 33),
                                  (96, 15), (96, 68), (96, 127), (1000, 15), (1000, 68)])
def test_b_group_sizes_and_sub_batches(n, nb, chain):
    names = _distinct_group(n, nb)
    assert len(names) == nb and len(set(names)) == nb
    for ch in (False, True):
        assert len({_oracle(nm, ch)["colsol"].tobytes() for nm in names}) == nb      # no two problems share an answer
    _solve_and_check(names, CHAIN if chain else WIDE, chain, tag=f"n={n} nb={nb}")


# ---- (c) slicing and order ----

def _c_lists():
    one = [_name(k, 300, s) for s in (0, 1) for k in (1, 2, 3, 4, 5, 8)][:11]
    by_size = {300: [_name(k, 300, 2) for k in (1, 2, 3, 5, 7)], 64: [_name(k, 64, 2) for k in (1, 2, 4, 6)],
               1000: [_name(k, 1000, 2) for k in (1, 2, 3)], 5: [_name(k, 5, 2) for k in (1, 5)]}
    # interleaved, not sorted by size (by_n is a std::map: the problems come back in input order only if the indices are kept right)
    order = [300, 64, 1000, 5, 300, 64, 300, 1000, 64, 5, 300, 1000, 64, 300]
    taken = {k: 0 for k in by_size}
    mixed = []
    for sz in order:
        mixed.append(by_size[sz][taken[sz]])
        taken[sz] += 1
    assert all(taken[k] == len(v) for k, v in by_size.items())
    return dict(one_group=one, mixed=mixed)


@pytest.mark.parametrize("chain", [False, True], ids=["wide", "chain"])
@pytest.mark.parametrize("which", ["one_group", "mixed"])
def test_c_slices_and_input_order(which, chain):
    names = _c_lists()[which]
    first = {}
    for order in (names, names[::-1]):
        for conc in (1, 2, 3, 4, 0):
            res = _solve_and_check(order, CHAIN if chain else WIDE, chain, tag=f"max_concurrent={conc}", max_concurrent=conc)
            for nm, b in zip(order, _bits(res)):
                assert first.setdefault(nm, b) == b, (nm, conc)              # the same bits in every slicing and order


# ---- (d) a failing problem does not touch its neighbours ----

def _poisoned(names, bad):
    """The group's matrices with ONE non-finite value in each problem of `bad` ({index: value}); the others are the pool's."""
    costs = [_cost(nm) for nm in names]
    for b, val in bad.items():
        c = costs[b].copy()
        n = len(c)
        c[n // 2, n // 3] = val
        costs[b] = c
    return costs


@pytest.mark.parametrize("chain", [False, True], ids=["wide", "chain"])
@pytest.mark.parametrize("n", [300, 2100])
@pytest.mark.parametrize("bad", [{2: np.nan, 4: np.inf}, {0: np.nan}, {5: np.inf}, {0: np.inf, 5: np.nan}, "in_17",
                                 {0: np.nan, 1: np.inf, 2: -np.inf, 3: np.nan, 4: np.inf, 5: np.nan}],
                         ids=["2_and_4", "first", "last", "first_and_last", "inside_a_sub_batch_of_17", "every_problem"])
def test_d_rejected_problems_leave_the_others_alone(n, bad, chain):
    # non-finite costs are the library's documented rejection: colred_partial raises a host-visible flag and no solver kernel runs
    # on that problem.  The call reports CYTO_ERR_NONFINITE; the healthy problems are the oracle's, counters included.
    if bad == "in_17":
        # G = 2 sub-batches, k % 2: problem 5 (NaN) is the third of the odd one, problem 10 (inf) the sixth of the even one
        names = [_name(k, n) for k in KINDS] + [_name(k, n) for k in KINDS] + [_name(1, n, 1)]
        names[9], names[11], names[13] = _name(1, n, 2), _name(5, n, 1), _name(8, n, 1)
        bad = {5: np.nan, 10: np.inf}
    else:
        names = [_name(k, n) for k in (1, 2, 3, 5, 8, 4)]
    opts = CHAIN if chain else WIDE
    costs = _poisoned(names, bad)
    with pytest.raises(ValueError, match="status 2"):
        lap_solve_batch(costs, return_info=True, opts=opts)
    outs, status = lap_solve_batch(costs, return_info=True, opts=opts, return_status=True)
    assert status == [NONFINITE if b in bad else 0 for b in range(len(names))]
    assert len(outs) == len(names)
    for b, (nm, g) in enumerate(zip(names, outs)):
        if b in bad:
            assert g is None
        else:
            _equals_oracle(g, nm, chain, tag=f"problem {b} beside rejected {sorted(bad)}")
    # and the same group, healthy, right behind the failure (whatever a rejected problem left in a cached buffer does not matter)
    _solve_and_check(names, opts, chain, tag="after the failure")


# ---- (e) costs already on the device ----

PAD = np.float32(-1e30)     # in every element of the buffer that is not a cost: a kernel that reads one changes the answer
NAN_PAD = np.float32(np.nan)   # ... and what a recycled block may hold: a NaN taken for a cost also fails the solve (CYTO_ERR_NONFINITE)


@pytest.mark.parametrize("chain", [False, True], ids=["wide", "chain"])
@pytest.mark.parametrize("layout", ["in_place", "odd_pitch", "offset_base", "odd_pitch_and_offset_base",
                                    "wide", "in_place_nan", "wide_nan", "odd_pitch_nan"])
@pytest.mark.parametrize("n", [301, 1000])
def test_e_costs_resident_on_the_device(n, layout, chain):
    # in_place: ld = n rounded up to 4 and a 16-byte aligned base, used where it lies; odd_pitch: ld = n + 1 (1000 -> 1001: rows not
    # 16-byte aligned); offset_base: the base 4 bytes into a larger allocation -- each of these goes through the device-to-device
    # re-pitch of lap_solve_f32_batch.  wide: ld = n rounded up to 4, plus 8 -- aligned, used in place, and wider than any padded
    # width (a kernel that steps rows by (n + 3) & ~3 instead of ld reads the wrong rows).  *_nan: NaN instead of -1e30
    names = [_name(k, n) for k in (1, 2, 3, 5, 8)]
    pad = NAN_PAD if layout.endswith("_nan") else PAD
    ld = n + 1 if "odd_pitch" in layout else (n + 3) // 4 * 4 + (8 if "wide" in layout else 0)
    lead = 1 if "offset_base" in layout else 0
    bufs = []

    def is_pad(a):
        return (a.view(np.uint32) == np.array([pad]).view(np.uint32)[0]).all()

    try:
        for nm in names:
            h = np.full(lead + n * ld + 3, pad, np.float32)
            h[lead:lead + n * ld].reshape(n, ld)[:, :n] = _cost(nm)
            bufs.append(_lib.DeviceBuffer.from_numpy(h))
        ptrs = [b.ptr + 4 * lead for b in bufs]
        assert all((p % 16 == 0) == (lead == 0) for p in ptrs)
        res = lap_solve_batch_device(ptrs, [n] * len(names), [ld] * len(names), return_info=True, opts=CHAIN if chain else WIDE)
        for b, (nm, g) in enumerate(zip(names, res)):
            _equals_oracle(g, nm, chain, tag=f"{layout} problem {b}")
        # the caller's buffers are read only
        for nm, buf in zip(names, bufs):
            back = buf.to_numpy((lead + n * ld + 3,), np.float32)
            assert np.array_equal(back[lead:lead + n * ld].reshape(n, ld)[:, :n], _cost(nm))
            assert is_pad(back[:lead]) and is_pad(back[lead + n * ld:])
            assert is_pad(np.ascontiguousarray(back[lead:lead + n * ld].reshape(n, ld)[:, n:]))
    finally:
        for b in bufs:
            b.free()


# ---- (f) row maps in a batch, through the context ----

@pytest.mark.parametrize("size", [240, 1200])
@pytest.mark.parametrize("K", [3, 17])
def test_f_row_maps_in_a_batch_through_the_context(K, size):
    """K same-size chunks in ONE assign_chunks call, every chunk with slot counts that repeat spots and leave others out (a row
    map with nused < n behind lap_batch_any's rowmap / nu).  Per chunk the reference is the wide oracle on the device's own cost rows
    of that chunk's cells and used spots (common.pearson_cost_device -> host -> rows[location_repeat]): this pins the batch's
    row-map plumbing, not the GEMM (test_cost_precision_gpu.py does that)."""
    from cytospace_amd import common
    from cytospace_amd.cytospace import ExpressionContext
    from tools import instances
    G, S = 200, 500
    C = K * size
    sc, st, _ = instances.synth_expression(G, C, S, seed=100 * K + size)
    rng = np.random.default_rng([K, size])
    chunks, maps = [], []
    for k in range(K):
        idx = np.sort(rng.permutation(C)[:size])
        nused = size // 3 + k                                   # (a different number of distinct rows in every chunk)
        used = np.sort(rng.permutation(S)[:nused])
        slots = np.zeros(S, np.int64)
        slots[used] = 1 + rng.multinomial(size - nused, np.full(nused, 1.0 / nused))
        assert slots.sum() == size and (slots > 1).any() and (slots == 0).any()
        chunks.append((idx, slots))
        maps.append(used)
    with ExpressionContext(sc, st, False) as ctx:
        got = ctx.assign_chunks(chunks, max_concurrent=K, return_info=True)
        sliced = ctx.assign_chunks(chunks, max_concurrent=max(2, K // 3))        # the context's own rounds of 2 / 5 chunks
    assert len(got) == K and len(sliced) == K
    assert all(np.array_equal(a[0], b) for a, b in zip(got, sliced))
    for k, ((idx, slots), used, (mapped, total, info)) in enumerate(zip(chunks, maps, got)):
        cost, N, ld, _ = common.pearson_cost_device(sc[:, idx], st[:, used], np.ones(len(used), np.int64), already_normalized=False)
        try:
            rows = cost.to_numpy((len(used), ld), np.float32)[:, :size]
        finally:
            cost.free()
        loc = np.repeat(np.arange(len(used)), slots[used])
        o = jv_oracle_wide(rows[loc], np.float32)
        assert np.array_equal(mapped, used[loc[o["colsol"]]]), k
        assert abs(total - o["total"]) <= 1e-5 * max(1.0, abs(o["total"])), (k, total, o["total"])
        gd, od = info.lap.as_dict(), o["stats"].as_dict()
        assert gd["wide"] == 1
        for kg, ko in WIDE_KEYS:
            assert gd[kg] == od[ko], (k, kg, gd[kg], od[ko])
        assert info.lap.row_groups == len(used), (k, info.lap.row_groups, len(used))      # the runs of the map


# ---- (g) options that claim not to matter, in a batch ----

_SINGLE_GAP = {}


@pytest.mark.parametrize("rounds", [0, 2])
@pytest.mark.parametrize("wipe", [0, 3])
@pytest.mark.parametrize("rebuild", [0, 1, -1])
def test_g_options_that_do_not_change_the_bits(rebuild, wipe, rounds):
    n = 2100
    names = [_name(k, n) for k in (1, 2, 3, 5)] + [_name(1, n, 1), _name(2, n, 1)]
    costs = [_cost(nm) for nm in names]
    for certify in (0, 1):
        opts = dict(mode=2, wide_rebuild=rebuild, wide_wipe=wipe, wide_rounds=rounds, certify=certify)
        res = lap_solve_batch(costs, return_info=True, opts=opts)
        for b, (nm, g) in enumerate(zip(names, res)):
            _equals_oracle(g, nm, False, rounds=rounds, tag=f"{opts} problem {b}")       # (the oracle with the same max_rounds)
            i = g["info"]
            assert i.certified == certify
            if certify:
                # the certificate is summed in a fixed order, the same bits on every run -- and in whatever company
                if (nm, rounds) not in _SINGLE_GAP:
                    s = lap_solve(costs[b], np.float32, return_info=True, opts=dict(mode=2, certify=1, wide_rounds=rounds))
                    _equals_oracle(s, nm, False, rounds=rounds, tag="single solve")
                    _SINGLE_GAP[(nm, rounds)] = (s["info"].gap_f64, s["info"].gap_max_f64, s["info"].gap_rows)
                assert (i.gap_f64, i.gap_max_f64, i.gap_rows) == _SINGLE_GAP[(nm, rounds)], (nm, opts)
                assert i.gap_f64 >= 0.0


# ---- (h) twice, and from two threads ----

@pytest.mark.parametrize("chain", [False, True], ids=["wide", "chain"])
def test_h_the_largest_group_twice_and_from_two_threads(chain):
    opts = CHAIN if chain else WIDE
    names = _distinct_group(1000, 33)
    a = _bits(_solve_and_check(names, opts, chain, tag="first call"))
    b = _bits(_solve_and_check(names, opts, chain, tag="second call"))
    assert a == b
    # two calls of 17 problems each at the same time: the sub-batch threads of both interleave on one device
    halves = [names[:17], names[16:]]
    assert all(len(h) == 17 for h in halves)
    costs = [[_cost(nm) for nm in h] for h in halves]
    out, errors = [None, None], []

    def run(t):
        try:
            out[t] = lap_solve_batch(costs[t], return_info=True, opts=opts)
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for t in range(2):
        for q, (nm, g) in enumerate(zip(halves[t], out[t])):
            _equals_oracle(g, nm, chain, tag=f"thread {t} problem {q}")
    assert _bits(out[0]) == a[:17] and _bits(out[1]) == a[16:]


# ---- (i) an option a batch does not have ----

def test_i_polish_is_refused_on_a_batch():
    # cyto_lap_opts.polish is the single-problem calls' (lap_solve_f32_one runs it behind the solve): a batch used to accept it and
    # return unpolished results with polished == 0.  Now CYTO_ERR_BAD_ARG for the call -- every problem's status too, nothing solved
    # -- and the next plain batch is the oracle's
    names = [_name(k, 300) for k in (1, 2, 3, 5)]
    costs = [_cost(nm) for nm in names]
    for opts in (dict(polish=1), dict(polish=1, mode=1), dict(polish=1, certify=1)):
        with pytest.raises(ValueError):
            lap_solve_batch(costs, return_info=True, opts=opts)
        with pytest.raises(ValueError):
            lap_solve_batch(costs, return_info=True, opts=opts, return_status=True)     # not a per-problem rejection: it raises as well
    _solve_and_check(names, None, False, tag="after the refused call")
    _solve_and_check(names, CHAIN, True, tag="after the refused call")
