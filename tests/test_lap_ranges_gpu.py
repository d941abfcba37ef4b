"""The float32 LAP kernels across the float range, against the CPU oracle bit for bit: costs scaled by 2^+-40 and 2^+-100, below the
normal range, with -0.0, with hundreds of binades inside one matrix (the pool of _ranges.py, gated by test_lap_ranges_cpu.py).

Every comparison is with the oracle OF THE MATRIX HANDED TO THE GPU (jv_oracle_wide for the wide solver and the default entry,
jv_oracle for the chain solver): rowsol, colsol, u, v with np.array_equal, WIDE_KEYS / STAT_KEYS, and `total` within
1e-12 * sum|c_assigned| of the oracle's (the same indices, the same addends, both summed in float64).  The suite's usual bound on the
total, 1e-5 * max(1, |total|), is an absolute 1e-5 for a small total and passes vacuously at 2^-100; the bound here is relative to the
addends.  That the oracle itself is right out there -- optimal against scipy, and inside the exact zone the base solve scaled -- is
test_lap_ranges_cpu.py's part and needs no GPU.

  (a) the wide solver (mode = 2) on every instance; in the exact zone wide_scaled and wide_phases also equal the BASE instance's GPU
      solve: the eps schedule does not move with the binade
  (b) the default entry (no options): the bits of (a)
  (c) the chain solver (mode = 1) on every instance with n <= 1000; at n = 300, k = +-100 also chain_variant 1, 2, 3 and the
      cache-certified search (augmentation = 2, no_handover = 1)
  (d) options that must not change a bit: wide_par, wide_rebuild, wide_wipe, cache_waves, cache_stream
  (e) a row map: kind 3 with every distinct row stored once
  (f) one batch of eight problems from eight corners of the range: whatever is per launch and should be per problem (eps, epsmin,
      thresholds) shows here
  (g) the work counters at k = -100, 0, 100, printed and not asserted (DESIGN.md has the table)

Time on an MI355X host, oracles included: 10 s for the 302 tests; the slowest are the three kind-2 instances at n = 2100, 0.7 s each.
"""
import numpy as np
import pytest

import _ranges
from cytospace_amd.lap import lap_solve, lap_solve_batch, lap_solve_rows
from test_lap_gpu import STAT_KEYS, WIDE_KEYS

pytestmark = pytest.mark.gpu

WIDE, CHAIN = dict(mode=2), dict(mode=1)
NAMES = _ranges.names()
_GPU = {}


def _equals_oracle(g, nm, chain, tag=""):
    c, o = _ranges.cost(nm), _ranges.oracle(nm, chain)
    n = len(c)
    for k in ("rowsol", "colsol", "u", "v"):
        assert np.array_equal(g[k], o[k]), (tag, nm, k)
    assigned = float(np.abs(c[np.arange(n), o["rowsol"]].astype(np.float64)).sum())
    assert abs(g["total"] - o["total"]) <= 1e-12 * assigned, (tag, nm, g["total"], o["total"])
    gd, od = g["info"].as_dict(), o["stats"].as_dict()
    assert gd["wide"] == (0 if chain else 1), (tag, nm)
    if chain:
        for k in STAT_KEYS:
            assert gd[k] == od[k], (tag, nm, k, gd[k], od[k])
    else:
        for kg, ko in WIDE_KEYS:
            assert gd[kg] == od[ko], (tag, nm, kg, gd[kg], od[ko])


def _solve(nm, chain):
    """The plain solve of an instance by one solver, checked against its oracle, once."""
    if (nm, chain) not in _GPU:
        g = lap_solve(_ranges.cost(nm), np.float32, return_info=True, opts=CHAIN if chain else WIDE)
        _equals_oracle(g, nm, chain)
        _GPU[(nm, chain)] = g
    return _GPU[(nm, chain)]


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("rowsol", "colsol", "u", "v")) and a["total"] == b["total"]


# ---- (a) the wide solver ----

@pytest.mark.parametrize("nm", NAMES)
def test_a_wide(nm):
    g = _solve(nm, False)
    if _ranges.is_exact_zone(nm) and _ranges.base_of(nm):
        b = _solve(_ranges.base_of(nm), False)
        assert (g["info"].wide_scaled, g["info"].wide_phases) == (b["info"].wide_scaled, b["info"].wide_phases)


# ---- (b) the default entry ----

@pytest.mark.parametrize("nm", [_ranges.name(kd, 300, k) for kd in (1, 2) for k in (-100, 100)] + ["subgrid-300"])
def test_b_default_entry(nm):
    g = lap_solve(_ranges.cost(nm), np.float32, return_info=True)
    _equals_oracle(g, nm, False, "no options")
    assert _same_bits(g, _solve(nm, False))


# ---- (c) the chain solver ----

@pytest.mark.parametrize("nm", [nm for nm in NAMES if _ranges.parts(nm)[1] <= 1000])
def test_c_chain(nm):
    _solve(nm, True)


@pytest.mark.parametrize("opts", [dict(chain_variant=1), dict(chain_variant=2), dict(chain_variant=3),
                                  dict(augmentation=2, no_handover=1)], ids=["variant1", "variant2", "variant3", "cache_certified"])
@pytest.mark.parametrize("nm", [_ranges.name(kd, 300, k) for kd in (1, 2) for k in (-100, 100)])
def test_c_chain_variants(nm, opts):
    g = lap_solve(_ranges.cost(nm), np.float32, return_info=True, opts=dict(CHAIN, **opts))
    _equals_oracle(g, nm, True, opts)
    assert _same_bits(g, _solve(nm, True))


# ---- (d) options that must not change a bit ----

@pytest.mark.parametrize("opts", [dict(wide_par=5), dict(wide_rebuild=1), dict(wide_wipe=3), dict(cache_waves=1), dict(cache_stream=-1)],
                         ids=lambda o: "%s=%d" % next(iter(o.items())))
@pytest.mark.parametrize("nm", ["kind2-1000-x2^-100", "kind2-1000-x2^100", "subgrid-1000"])
def test_d_options_that_do_not_change_the_bits(nm, opts):
    g = lap_solve(_ranges.cost(nm), np.float32, return_info=True, opts=dict(WIDE, **opts))
    _equals_oracle(g, nm, False, opts)
    assert _same_bits(g, _solve(nm, False))


# ---- (e) a row map ----

@pytest.mark.parametrize("chain", [False, True], ids=["wide", "chain"])
@pytest.mark.parametrize("k", [-100, 100])
@pytest.mark.parametrize("n", [300, 1000])
def test_e_row_map(n, k, chain):
    nm = _ranges.name(3, n, k)
    c = _ranges.cost(nm)
    rows, rowmap = np.ascontiguousarray(c[::4]), (np.arange(n) // 4).astype(np.int32)
    assert np.array_equal(rows[rowmap], c)                          # every distinct row once
    g = lap_solve_rows(rows, rowmap, return_info=True, opts=CHAIN if chain else WIDE)
    _equals_oracle(g, nm, chain, "row map")
    assert g["info"].row_groups == n // 4


# ---- (f) one batch, many binades ----

@pytest.mark.parametrize("chain", [False, True], ids=["wide", "chain"])
@pytest.mark.parametrize("n", [96, 300])
def test_f_one_batch_many_binades(n, chain):
    names = _ranges.batch_group(n)
    assert len(names) == 8
    res = lap_solve_batch([_ranges.cost(nm) for nm in names], return_info=True, opts=CHAIN if chain else WIDE)
    assert len(res) == 8
    for b, (nm, g) in enumerate(zip(names, res)):
        _equals_oracle(g, nm, chain, f"problem {b} of the batch")


# ---- (g) work done: recorded, not asserted ----

@pytest.mark.parametrize("n,kind", [(1000, 1), (1000, 2), (2100, 1), (2100, 2), (1000, 3), (1000, 5), (1000, 8)])
def test_g_work_counters_across_scales(n, kind):
    # wide_dense_arr / wide_dense_aug: bids / relaxations the row caches could not certify (the whole row was read instead).  The
    # cache builders hold two absolute constants (delta = 1e-3f for a tied row, 1e30f as "no delta"); if they cost anything far from 1,
    # it shows here.  Kinds 1 and 2 are the table of DESIGN.md; 3, 5 (tied rows) and 8 (large values) are what the constants touch
    for k in (-100, 0, 100):
        i = _solve(_ranges.name(kind, n, k), False)["info"]
        print(f"kind {kind} n={n} k={k:+4d}: wide_dense_arr {i.wide_dense_arr} wide_dense_aug {i.wide_dense_aug} "
              f"hbm_row_reads {i.hbm_row_reads} wide_aug_launches {i.wide_aug_launches}")
