"""The claim rule of the several-searches-at-once kernel (lap_wide.hip: search_end), as a pure-Python model.

Every search g of a batch claims its columns with a RETURNING atomic max of (batch << 8 | 255 - g).  Of the word that comes back: if
its batch field is this batch's and its workgroup field is another search's, the two share the column, and the one with the larger g is
flagged (an atomic min into P).  Whatever the order in which the individual claims arrive, the flagged set must be
{g : g shares a column with some g' < g} -- what a check pass behind a grid barrier found before -- and P its minimum."""
import itertools
import random

import pytest

GMAX = 64
NO_CONFLICT = GMAX + 1


def run_batch(claim, batch, arrivals, G):
    """arrivals: (g, column) in the order the atomics reach memory.  Returns (flagged set, P)."""
    flagged, P = set(), NO_CONFLICT
    for g, k in arrivals:
        key = (batch << 8) | (255 - g)
        old = claim.get(k, 0)
        claim[k] = max(old, key)                                   # the atomic max ...
        if (old >> 8) == batch and old != key:                     # ... and the word it returned
            go = 255 - (old & 255)
            flagged.add(max(g, go))
            P = min(P, max(g, go))
    assert all(0 <= g < G for g in flagged)
    return flagged, P


def expected(sets):
    out = set()
    for g, cols in enumerate(sets):
        if any(cols & sets[h] for h in range(g)):
            out.add(g)
    return out


def random_family(rng, G, ncols, density):
    return [set(k for k in range(ncols) if rng.random() < density) | {rng.randrange(ncols)} for _ in range(G)]


def orders(rng, sets):
    """Arrival orders of the individual claims: random ones, search by search upwards and downwards (the lowest search arrives
    last), and interleaved column by column in both directions."""
    claims = [(g, k) for g, cols in enumerate(sets) for k in sorted(cols)]
    yield list(claims)
    yield sorted(claims, key=lambda c: (-c[0], c[1]))              # the lowest search arrives last
    yield sorted(claims, key=lambda c: (c[1], c[0]))
    yield sorted(claims, key=lambda c: (c[1], -c[0]))              # per column: the lowest claimant last
    for _ in range(6):
        o = list(claims)
        rng.shuffle(o)
        yield o


@pytest.mark.parametrize("G", [2, 5, 16])
def test_flagged_set_whatever_the_order(G):
    rng = random.Random(1000 + G)
    seen_multi, seen_conflict_free = False, False
    for trial in range(60):
        ncols = rng.choice([4, 12, 40, 200])
        if trial % 10 == 0:                                        # pairwise disjoint: the batch commits whole
            sets = [{3 * g, 3 * g + 1 + trial % 2} for g in range(G)]
            ncols = 3 * G
        else:
            sets = random_family(rng, G, ncols, rng.choice([0.02, 0.1, 0.3]))
        want = expected(sets)
        seen_multi = seen_multi or any(sum(k in s for s in sets) >= 3 for k in range(ncols))
        seen_conflict_free = seen_conflict_free or not want
        for arr in orders(rng, sets):
            flagged, P = run_batch({}, 7, arr, G)
            assert flagged == want, (G, trial, sets)
            assert P == (min(want) if want else NO_CONFLICT)
    assert seen_conflict_free and (seen_multi or G == 2)           # columns with three and more claimants; batches that commit whole


def test_every_order_of_a_column_with_three_claimants():
    # searches 0, 1, 3 share column 5; search 2 is on its own: flagged {1, 3} in all 4! orders of the four claims
    base = [(0, 5), (1, 5), (3, 5), (2, 9)]
    for arr in itertools.permutations(base):
        flagged, P = run_batch({}, 3, list(arr), 4)
        assert flagged == {1, 3} and P == 1


def test_stale_words_flag_nobody():
    rng = random.Random(5)
    claim = {}
    for batch in range(1, 40):
        G = rng.choice([2, 5, 16])
        if batch % 2:
            sets = [{g} for g in range(G)]                         # disjoint sets over columns every earlier batch has claimed
        else:
            sets = random_family(rng, G, 16, 0.2)
        arr = [(g, k) for g, cols in enumerate(sets) for k in cols]
        rng.shuffle(arr)
        flagged, P = run_batch(claim, batch, arr, G)               # (claim carries the words of all earlier batches)
        assert flagged == expected(sets)
        if batch % 2:
            assert not flagged and P == NO_CONFLICT
    # a word of the batch before with a LOWER workgroup field than the arrival's: still nobody
    claim = {3: (8 << 8) | 255}
    assert run_batch(claim, 9, [(4, 3)], 16) == (set(), NO_CONFLICT)
    assert claim[3] == (9 << 8) | (255 - 4)


def test_the_sink_is_a_claim_like_any_other():
    # search 1 ends at a column search 0 settled; search 2 settled search 1's sink
    sets = [{10, 11}, {12} | {10}, {20} | {12}]
    for arr in itertools.permutations([(g, k) for g, cols in enumerate(sets) for k in cols]):
        flagged, P = run_batch({}, 2, list(arr), 3)
        assert flagged == {1, 2} and P == 1
