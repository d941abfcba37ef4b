"""Ending a search that can no longer be committed (lap_wide.hip: wide_aug<.., PAR>), as pure-Python models.

Group 1, the batch: every search may send some of its claims EARLY (columns it is certain to settle), polls P before every step and
is aborted -- no further claim, no end -- once P <= g or a claim of its own flags it.  Whatever the interleaving, P and with it the
committed prefix must be those of the rule that claims at the ends only (tests/test_par_claims_cpu.py), and nobody below that P is
ever aborted.  (The kernel polls and aborts; it sends no early claims -- the model with an empty list of them is the kernel's rule,
and the edge cases below run it both ways.)

Group 2, which columns are certain -- the rule early claims would have to obey (built, exact, too dear in its first form,
not in the kernel): a label-correcting search in rounds over a small graph with ties (zero-weight edges: the hop
count orders them) and truncated adjacency (a row's cache holds its K cheapest edges, the rest only has a floor and is relaxed when
the verify pass finds the floor too low).  A picked column whose distance is strictly below B (the round minima of the dirty
distances, this round's and the one before because a block that was picked from is invisible for a round), below F (the floors of
everything processed so far and of the root) and below the best unassigned distance must lie in the final settled set.  The test
also drops B and F in turn and demands that the model then certifies a column it should not have: the conditions are needed."""
import random

import pytest

GMAX = 64
NO_CONFLICT = GMAX + 1


# ---------------------------------------------------------------- group 1: the batch

def end_only_P(sets):
    flagged = [g for g, cols in enumerate(sets) if any(cols & sets[h] for h in range(g))]
    return min(flagged) if flagged else NO_CONFLICT


def run_batch(sets, early, order, batch=5, poll=True):
    """sets[g]: settled columns and sink of search g.  early[g]: the claims g sends before its end, in order (duplicates allowed).
    order: a sequence of g -- whose next step happens (steps of g: its early claims, then its end, which claims all of sets[g]).
    Returns (P, aborted set)."""
    claim, P, aborted = {}, NO_CONFLICT, set()
    pos = [0] * len(sets)

    def send(g, k):
        nonlocal P
        key = (batch << 8) | (255 - g)
        old = claim.get(k, 0)
        claim[k] = max(old, key)
        if (old >> 8) == batch and old != key:
            f = max(g, 255 - (old & 255))
            P = min(P, f)
            return f == g
        return False

    for g in order:
        if g in aborted or pos[g] > len(early[g]):
            continue
        if poll and P <= g:                                        # the poll of the round
            aborted.add(g)
            continue
        if pos[g] < len(early[g]):
            k = early[g][pos[g]]
            assert k in sets[g]                                    # (only certain columns are claimed early)
            if send(g, k):
                aborted.add(g)                                     # flagged itself: P <= g now
                assert P <= g
        else:
            for k in sorted(sets[g]):
                send(g, k)                                         # the end: every column, flags as before, nothing to abort
        pos[g] += 1
    assert all(g in aborted or pos[g] == len(early[g]) + 1 for g in range(len(sets)))
    return P, aborted


def orders(rng, steps):
    """Interleavings of the searches' steps: random, lowest search first / last, round-robin."""
    G = len(steps)
    flat = [g for g in range(G) for _ in range(steps[g])]
    yield list(flat)
    yield list(reversed(flat))
    rr, left = [], list(steps)
    while any(left):
        for g in range(G):
            if left[g]:
                rr.append(g); left[g] -= 1
    yield rr
    yield list(reversed(rr))
    for _ in range(8):
        o = list(flat)
        rng.shuffle(o)
        yield o


def check_family(rng, sets):
    want = end_only_P(sets)
    G = len(sets)
    for it in range(4):
        early = []
        for g in range(G):
            cols = sorted(sets[g])
            e = [k for k in cols if rng.random() < 0.5 and it > 0]    # (the first pass: no early claims, the poll alone)
            e += [rng.choice(cols) for _ in range(rng.randrange(3) if it > 0 else 0)]          # duplicate claims
            rng.shuffle(e)
            early.append(e)
        for order in orders(rng, [len(e) + 1 for e in early]):
            P, aborted = run_batch(sets, early, order)
            assert P == want, (sets, early, order, P, want)
            assert min(P, G) == min(want, G)                       # the committed prefix
            assert all(g >= want for g in aborted), (sets, aborted, want)


@pytest.mark.parametrize("G", [2, 5, 16])
def test_p_and_prefix_equal_the_end_only_rule(G):
    rng = random.Random(2000 + G)
    seen = set()
    for trial in range(40):
        ncols = rng.choice([4, 12, 40, 200])
        dens = rng.choice([0.02, 0.1, 0.3])
        sets = [set(k for k in range(ncols) if rng.random() < dens) | {rng.randrange(ncols)} for _ in range(G)]
        seen.add(end_only_P(sets) == NO_CONFLICT)
        check_family(rng, sets)
    assert seen == {True, False} or G == 16                        # batches that commit whole and batches that do not


def test_edge_cases():
    rng = random.Random(7)
    check_family(rng, [{3} | {10 + g} for g in range(16)])         # all searches share one column: P = 1
    check_family(rng, [{3}] * 5)
    check_family(rng, [{2 * g, 2 * g + 1} for g in range(16)])     # nobody shares: P = no conflict, nobody aborted
    for early in ([[], [], []], [[1, 1], [2], [3, 3, 3]]):
        P, aborted = run_batch([{1}, {2}, {3}], early, [0, 1, 2] * 4)
        assert P == NO_CONFLICT and not aborted
    # the lowest flagged search (1) is aborted -- by its own early claim of column 6 -- before it ever claims column 5, which it
    # shares with search 0 too; search 2 shares column 9 with search 1 only and is aborted by the poll.  P = 1 all the same.
    sets = [{5, 6}, {5, 6, 9}, {9}]
    P, aborted = run_batch(sets, [[], [6, 5], []], [0, 1, 1, 1, 2, 2])
    assert P == 1 and aborted == {1, 2}
    # ... and when search 1's early claim arrives first, search 0's end flags it: search 1 sees it at its next poll
    P, aborted = run_batch(sets, [[], [6, 5], []], [1, 0, 1, 1, 2, 2])
    assert P == 1 and aborted == {1, 2}
    # duplicate claims with the same key flag nobody
    P, aborted = run_batch([{4}, {8}], [[4, 4, 4], [8, 8]], [0, 0, 0, 0, 1, 1, 1])
    assert P == NO_CONFLICT and not aborted


def test_without_the_poll_the_claims_alone_keep_p():
    # (the poll only ends searches sooner: early claims without it give the same P)
    rng = random.Random(11)
    for trial in range(30):
        sets = [set(k for k in range(12) if rng.random() < 0.2) | {rng.randrange(12)} for _ in range(5)]
        early = [[k for k in sorted(s) if rng.random() < 0.5] for s in sets]
        for order in orders(rng, [len(e) + 1 for e in early]):
            assert run_batch(sets, early, order, poll=False)[0] == end_only_P(sets)


# ---------------------------------------------------------------- group 2: which columns are certain

INF = (1 << 30, 0)


def edge_label(d, h, w):
    return (d + w, 0) if w > 0 else (d, h + 1)                     # (edge_lv: a tight edge keeps the distance and counts a hop)


def search(rng, n_asg, n_free, K, wmax, use_B=True, use_F=True, picks=3, nblocks=4):
    """One search on a random instance.  Returns (certified columns, final settled set)."""
    ncol = n_asg + n_free                                          # columns 0 ... n_asg - 1 are assigned (column k is owned by row k)
    # row n_asg: the free row (the root); the unassigned columns are some way off from most rows, so that the search goes deep, and
    # close to a few, so that the end can still fall late
    far = rng.choice([wmax, 2 * wmax, 3 * wmax])
    rows = [[rng.randrange(wmax + 1) + (far if c >= n_asg and rng.random() < 0.8 else 0) for c in range(ncol)] for _ in range(n_asg + 1)]
    for k in range(n_asg):
        rows[k][k] = None                                          # (a row offers nothing to its own column)

    def cache_of(i):
        cand = sorted((w, c) for c, w in enumerate(rows[i]) if w is not None)
        return cand[:K], (cand[K][0] if len(cand) > K else 1 << 29)                          # cached edges, floor of the rest
    caches = [cache_of(i) for i in range(n_asg + 1)]
    label = [INF] * ncol
    dirty, dense = set(), set()
    T = [INF]
    root = n_asg

    def offer(c, lv):
        if lv < label[c] and lv <= T[0]:
            label[c] = lv
            if c < n_asg:
                dirty.add(c)
            else:
                T[0] = min(T[0], lv)

    for w, c in caches[root][0]:
        offer(c, (w, 0))
    F = caches[root][1]
    b1 = b2 = 0
    block = lambda c: c % nblocks
    invisible = set()
    pending, certified = [], set()
    rootdense = False
    while True:
        while True:                                                # the rounds
            lim = T[0][0]
            if use_B:
                lim = min(lim, b1, b2)
            if use_F:
                lim = min(lim, F)
            for k, d in pending:
                if d < lim:
                    certified.add(k)
            elig = [c for c in dirty if label[c] < T[0]]
            vis = [c for c in elig if block(c) not in invisible]
            b_now = min([label[c][0] for c in vis], default=1 << 30)
            rng.shuffle(vis)
            picked = vis[:picks]
            was_invisible = bool(invisible)
            invisible = {block(c) for c in picked}
            for k in picked:
                dirty.discard(k)
            for k in picked:                                       # (labels are read after the dirty bits are cleared)
                d, h = label[k]
                if (d, h) >= T[0]:
                    continue
                pending.append((k, d))
                if k in dense:
                    for c, w in enumerate(rows[k]):
                        if w is not None:
                            offer(c, edge_label(d, h, w))
                else:
                    F = min(F, d + caches[k][1])
                    for w, c in caches[k][0]:
                        offer(c, edge_label(d, h, w))
            b2, b1 = b1, b_now
            if not picked and not was_invisible and not invisible:
                break
        fail = False                                               # converged: do the caches certify what was skipped?
        for k in range(n_asg):
            if label[k] < T[0] and k not in dense and not (label[k][0] + caches[k][1] > T[0][0]):
                dense.add(k); dirty.add(k); fail = True
        if not rootdense and not (caches[root][1] > T[0][0]):
            rootdense = True; fail = True
            for c, w in enumerate(rows[root]):
                offer(c, (w, 0))
        if not fail:
            break
        b1 = b2 = 0
    settled = {k for k in range(n_asg) if label[k] < T[0]}
    return certified, settled


def sweep(seed, **kw):
    bad = total = 0
    for trial in range(400):
        rng = random.Random(seed * 100003 + trial)
        n_asg = rng.choice([6, 10, 16, 40])
        # (K = 99: every edge is cached, F never binds -- the uniform instances; K = 1 ... 3: most edges are not -- few cell types)
        cert, settled = search(rng, n_asg, rng.choice([1, 2, 4]), rng.choice([1, 2, 3, 99]), rng.choice([1, 2, 4]), **kw)
        total += len(cert)
        bad += len(cert - settled)
    return bad, total


def test_certified_columns_are_settled_at_the_end():
    bad, total = sweep(1)
    assert bad == 0 and total > 0                                  # (and the rule does certify columns: the check is not vacuous)


def test_both_conditions_are_needed():
    assert sweep(1, use_B=False)[0] > 0                            # without B: a column still to be relabelled, or one the end falls below
    assert sweep(1, use_F=False)[0] > 0                            # without F: an uncached edge found by the verify pass lowers the end
