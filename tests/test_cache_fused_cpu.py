"""The first row caches from the column reduction's own pass (cytospace_amd/csrc/lap_jv.hip: colred_partial_append, fused_w,
fused_theta and fused_fixup), restated step by step in numpy:

  1. w[j]: the minimum of column j over the first RS = min(1024, n / 2) rows -- an upper bound of the final price v[j];
  2. theta[i]: lane l of a wave owns the quads l, l + 64, ... of the row's first 2 048 columns; the (i0 + 1)-th smallest of the 64 lane
     minima of fl(c - w), i0 = 64 (1 - exp(-(c0 + 1) / 64)), c0 = clamp(190 * 2048 / n, 6, 49);
  3. the list of row i: every column with fl(c - w[j]) < theta[i], in ANY order, counted past its 512 entries;
  4. the fix-up against the final prices: h = fl(raw - v[col]); 63 or fewer below theta: tau = theta, else tau = the 64th smallest h
     (found on order-preserving keys, bit by bit, as the kernel does); kept on strict '<'; a row fails over 512 listed columns or
     under min_kept(n) kept ones -- half of what theta aims at below it, 16 at least and 48 from 4 096 columns on (the row
     reduction pays for thin caches with full-row bids: lap_jv.hip).

What is pinned is the INVARIANT the solvers' exactness rests on: the cache of every row that does not fail is exactly
{ j : fl(c - v[j]) < tau }, 16 ... 63 columns sorted by column -- whatever w >= v is, and whatever the order of the list.  The kernels
themselves: tests/test_cache_fused_gpu.py."""
import numpy as np
import pytest

KCU, CAP, S, TARGET = 63, 512, 2048, 190


def f2ord(h):
    b = (np.asarray(h, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def ord2f(o):
    o = np.uint32(o)
    return np.array([o ^ np.uint32(0x80000000) if o & np.uint32(0x80000000) else ~o], np.uint32).view(np.float32)[0]


def min_kept(n):
    c0 = min(49.0, max(6.0, TARGET * S / n))
    return int(min(48.0, max(16.0, 0.5 * c0 * n / S)))


def sampled_w(c):
    n = c.shape[1]
    return c[:min(1024, n // 2)].min(axis=0)


def thetas(c, w):
    """theta of every row of c (rows x n, n >= 2 048)"""
    rows, n = c.shape
    assert n >= S
    d = (c[:, :S] - w[:S]).reshape(rows, S // 256, 64, 4)           # quad q = 64 u + lane holds the columns 4 q ... 4 q + 3
    lane_min = d.min(axis=(1, 3))
    c0 = min(49.0, max(6.0, TARGET * S / n))
    i0 = int(np.float32(64.0) * (np.float32(1.0) - np.exp(np.float32(-(c0 + 1.0) * 0.015625))))
    return np.sort(lane_min, axis=1)[:, i0]


def kth_smallest_key(keys, k):
    """the largest P with at most k keys below it, built from the top bit down: the (k + 1)-th smallest key"""
    P = np.uint32(0)
    for bit in range(31, -1, -1):
        cand = P | np.uint32(1 << bit)
        if np.count_nonzero(keys < cand) <= k:
            P = cand
    return P


def fixup(row, v, theta, listed, n):
    """(ok, tau, cache columns) for one row from its list of column indices (any order)"""
    if len(listed) > CAP:
        return False, theta, []
    listed = np.asarray(listed, np.int64)
    raw = row[listed]
    h = raw - v[listed]
    h = np.where(h < theta, h, np.float32(np.inf))
    tau = theta
    if np.count_nonzero(h < np.inf) > KCU:
        tau = ord2f(kth_smallest_key(f2ord(h), KCU))
        assert tau == np.sort(h)[KCU]                                # (the bitwise search finds the 64th smallest)
    kept = listed[h < tau]
    if len(kept) < min_kept(n) and n > 16:
        return False, tau, []
    return True, tau, sorted(kept.tolist())


def check_rows(c, v, w, rows, rng=None):
    """the invariant on the given rows; returns (rows that failed, sizes of the caches of the others)"""
    n = c.shape[1]
    assert np.all(w >= v)
    th = thetas(c[rows], w)
    failed, sizes = 0, []
    for k, i in enumerate(rows):
        listed = np.flatnonzero(c[i] - w < th[k])                    # step 3: the kernel appends them in whatever order its waves arrive
        ok, tau, cols = fixup(c[i], v, th[k], listed, n)
        if rng is not None and len(listed) <= CAP:                   # the order of the list changes nothing
            ok2, tau2, cols2 = fixup(c[i], v, th[k], rng.permutation(listed), n)
            assert (ok2, cols2) == (ok, cols) and (not ok or tau2 == tau)
        if not ok:
            failed += 1
            continue
        assert tau <= th[k]
        assert cols == np.flatnonzero(c[i] - v < tau).tolist()        # EVERY column below the floor, and nothing else
        assert 16 <= min_kept(n) <= len(cols) <= KCU
        sizes.append(len(cols))
    return failed, sizes


def overflow_cost(n, seed=11):
    """Uniform rows, but every 16th row (i % 16 == 5) is large in its first 2 048 columns and tiny behind them: far more than 512 columns
    lie below any threshold the large part gives, the list overflows and the row fails.  A row of only 2 304 columns has 256 columns
    behind the first 2 048 -- too few to overflow a 512-entry list -- so the quads of the lanes 0 ... 33 of the first 2 048 columns
    are tiny too (the 35th smallest lane minimum is then one of the large values at every n)."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, n)).astype(np.float32)
    odd = np.arange(n) % 16 == 5
    big = (5.0 + rng.random((int(odd.sum()), n))).astype(np.float32)
    tiny = (rng.random((int(odd.sum()), n)) * 1e-3).astype(np.float32)
    col = np.arange(n)
    tiny_cols = (col >= S) | ((col // 4) % 64 < 34)
    c[odd] = np.where(tiny_cols, tiny, big)
    return c


@pytest.mark.parametrize("n", [2048, 2051, 4999])
def test_uniform_rows_are_certified(n):
    rng = np.random.default_rng(n)
    c = rng.random((n, n)).astype(np.float32)
    v, w = c.min(axis=0), sampled_w(c)
    rows = np.concatenate([np.arange(0, 64), rng.integers(0, n, 192)])
    failed, sizes = check_rows(c, v, w, rows, rng)
    assert failed <= len(rows) // 8 and np.mean(sizes) >= 40       # (n = 2 048: ~49 columns lie below theta against w, fewer against v)


def test_uniform_rows_n20000():
    # the matrix in blocks of rows (1.6 GB at once otherwise): the prices need every row, the rows checked come from the first block
    n, blk = 20000, 1000
    rng = np.random.default_rng(20000)
    first = rng.random((blk, n), dtype=np.float32)
    w = np.minimum(first.min(axis=0), rng.random((24, n), dtype=np.float32).min(axis=0))     # rows 0 ... 1 023
    v = w.copy()
    for r in range(1024, n, blk):
        v = np.minimum(v, rng.random((min(blk, n - r), n), dtype=np.float32).min(axis=0))
    failed, sizes = check_rows(first, v, w, np.arange(0, 256), rng)
    assert failed == 0 and np.mean(sizes) >= 56


def test_few_levels_and_integer_ties():
    rng = np.random.default_rng(5)
    n = 2100
    # integer costs 0 ... 9: no threshold separates the ties; every row fails or holds exactly the columns below its floor
    c = rng.integers(0, 10, (n, n)).astype(np.float32)
    failed, _ = check_rows(c, c.min(axis=0), sampled_w(c), np.arange(0, n, 7), rng)
    assert failed == len(range(0, n, 7))
    # a few-cell-type matrix: rows and columns of six types; the sampled minima lie far above the final ones for most columns
    types = 6
    prof = rng.normal(size=(types, 64)).astype(np.float32)
    r = prof[rng.integers(0, types, n)] + 0.05 * rng.normal(size=(n, 64)).astype(np.float32)
    q = prof[rng.integers(0, types, n)] + 0.05 * rng.normal(size=(n, 64)).astype(np.float32)
    c = -(r @ q.T).astype(np.float32)
    check_rows(c, c.min(axis=0), sampled_w(c), np.arange(0, n, 7), rng)


@pytest.mark.parametrize("n", [2304, 4999])
def test_overflowing_lists_fail(n):
    c = overflow_cost(n)
    v, w = c.min(axis=0), sampled_w(c)
    odd = np.flatnonzero(np.arange(n) % 16 == 5)[:24]
    th = thetas(c[odd], w)
    assert all(np.count_nonzero(c[i] - w < t) > CAP for i, t in zip(odd, th))
    failed, _ = check_rows(c, v, w, odd)
    assert failed == len(odd)
    rest = np.flatnonzero(np.arange(n) % 16 != 5)[:240]
    failed, sizes = check_rows(c, v, w, rest, np.random.default_rng(1))
    assert failed <= len(rest) // 16 and min(sizes) >= 16


def test_any_upper_bound_of_the_prices_is_exact():
    n = 2500
    rng = np.random.default_rng(77)
    c = rng.random((n, n)).astype(np.float32)
    v = c.min(axis=0)
    rows = np.arange(0, n, 25)
    failed, sizes = check_rows(c, v, v.copy(), rows, rng)           # w == v: the list IS the set below theta
    assert failed == 0 and np.mean(sizes) >= 56
    far = v + np.float32(0.5)                                       # w far above v: short lists, small caches or failures, never a wrong cache
    check_rows(c, v, far, rows, rng)
    mixed = np.where(np.arange(n) % 3 == 0, v, far)
    check_rows(c, v, mixed, rows, rng)
