"""One conflict flag per wave (lap_wide.hip: search_end<.., PAR>), as a pure-Python model beside tests/test_par_claims_cpu.py.

Every search g of a batch claims its settled columns and its sink with a RETURNING atomic max of (batch << 8 | 255 - g); of the word
that comes back, the larger g of the pair is flagged.  The kernel does not send every flag to P: a THREAD keeps the lowest flagged g
it has seen -- its own search's or the other claimant's -- in a register, and behind the pass a WAVE that saw a flag sends one atomic
min.  P must be what one atomic min per flagged column gave: the lowest search that shares a column with a lower one, or "no
conflict" -- whatever the order in which the claims arrive and however a search's columns are dealt to its threads and waves."""
import itertools
import random

import pytest

GMAX = 64
NO_CONFLICT = GMAX + 1
WAVE = 64


def p_per_column(batch, arrivals):
    """The rule before: an atomic min into P for every flagged claim.  arrivals: (g, column, thread) in the order the atomics reach memory."""
    claim, P = {}, NO_CONFLICT
    for g, k, _ in arrivals:
        key = (batch << 8) | (255 - g)
        old = claim.get(k, 0)
        claim[k] = max(old, key)
        if (old >> 8) == batch and old != key:
            P = min(P, max(g, 255 - (old & 255)))
    return P


def p_per_wave(batch, arrivals, threads, claim=None):
    """The kernel's rule (claim: the claim words earlier batches left).  Returns (P, atomics sent to P, some flag named the OTHER
    claimant, flagged claims)."""
    claim = {} if claim is None else claim
    fmin = {}                                                       # (g, thread) -> the register
    other, nflags = False, 0
    for g, k, t in arrivals:
        assert 0 <= t < threads
        key = (batch << 8) | (255 - g)
        old = claim.get(k, 0)
        claim[k] = max(old, key)
        if (old >> 8) == batch and old != key:
            go = 255 - (old & 255)
            other = other or go > g
            nflags += 1
            fmin[(g, t)] = min(fmin.get((g, t), NO_CONFLICT), max(g, go))
    waves = {}
    for (g, t), f in fmin.items():                                  # the wave reduction
        waves[(g, t // WAVE)] = min(waves.get((g, t // WAVE), NO_CONFLICT), f)
    P, sent = NO_CONFLICT, 0
    for f in waves.values():                                        # a wave that saw none sends nothing
        assert f <= GMAX
        P = min(P, f); sent += 1
    return P, sent, other, nflags


def expected_p(sets):
    for g, cols in enumerate(sets):
        if any(cols & sets[h] for h in range(g)):
            return g
    return NO_CONFLICT


def deal(rng, sets, sinks, threads, how):
    """The claims of a batch with the thread that makes each: how = 'kernel' (the touched list striped over the workgroup, four
    columns per thread and trip; the sink by thread 0), 'one' (everything on one thread), 'random'."""
    out = []
    for g, cols in enumerate(sets):
        settled = sorted(cols - {sinks[g]})
        rng.shuffle(settled)
        for q, k in enumerate(settled):
            t = q % threads if how == "kernel" else 0 if how == "one" else rng.randrange(threads)
            out.append((g, k, t))
        out.append((g, sinks[g], 0 if how != "random" else rng.randrange(threads)))
    return out


def orders(rng, claims, nrandom=4):
    yield list(claims)
    yield sorted(claims, key=lambda c: (-c[0], c[1]))               # the lowest search arrives last: it flags the others
    yield sorted(claims, key=lambda c: (c[1], c[0]))
    yield sorted(claims, key=lambda c: (c[1], -c[0]))
    for _ in range(nrandom):
        o = list(claims)
        rng.shuffle(o)
        yield o


def family(rng, G, ncols, sizes):
    sets, sinks = [], []
    for g in range(G):
        cols = set(rng.sample(range(ncols), min(sizes[g % len(sizes)], ncols - 1)))
        sink = rng.choice([k for k in range(ncols) if k not in cols] or [0])
        sets.append(cols | {sink}); sinks.append(sink)
    return sets, sinks


@pytest.mark.parametrize("G", [2, 5, 16])
def test_one_minimum_per_wave_is_one_minimum_per_column(G):
    rng = random.Random(2000 + G)
    seen_other, seen_free, seen_fewer = False, False, False
    for trial in range(40):
        sizes = rng.choice([[0, 1, 63, 64, 65], [65, 64, 63, 1, 0], [1], [63, 65], [0], [200, 3]])
        ncols = rng.choice([80, 130, 400])
        if trial % 8 == 0:                                          # pairwise disjoint: no flag at all
            sets = [{3 * g, 3 * g + 1} for g in range(G)]
            sinks = [3 * g for g in range(G)]
        else:
            sets, sinks = family(rng, G, ncols, sizes)
        want = expected_p(sets)
        seen_free = seen_free or want == NO_CONFLICT
        for how in ("kernel", "one", "random"):
            for threads in (64, 1024):
                claims = deal(rng, sets, sinks, threads, how)
                for arr in orders(rng, claims):
                    assert p_per_column(7, arr) == want
                    P, sent, other, nflags = p_per_wave(7, arr, threads)
                    assert P == want, (G, trial, how, threads)
                    assert sent <= G * (threads // WAVE)
                    if want == NO_CONFLICT:
                        assert sent == 0                            # P stays "no conflict": nobody writes it
                    seen_other = seen_other or other
                    assert sent <= nflags
                    seen_fewer = seen_fewer or sent < nflags        # many flags, fewer atomics
    assert seen_other and seen_free and seen_fewer


def test_a_few_thousand_columns_per_search():
    # a deep search that shares thousands of columns with a lower one: 16 atomics at the most from its workgroup, the same P
    rng = random.Random(9)
    ncols = 6000
    sets, sinks = family(rng, 5, ncols, [3892, 2210, 1664, 10, 0])
    want = expected_p(sets)
    assert want == 1 and len(sets[0] & sets[1]) > 1024
    for how in ("kernel", "random"):
        claims = deal(rng, sets, sinks, 1024, how)
        for arr in orders(rng, claims, nrandom=2):
            P, sent, _, nflags = p_per_wave(3, arr, 1024)
            assert P == want == p_per_column(3, arr)
            assert sent <= 5 * 16 and nflags > 1024


def test_every_order_and_every_split_of_a_small_batch():
    # searches 0, 1, 3 share column 5, search 2 ends (its sink) at a column search 1 settled: P = 1 in every order, on every
    # assignment of the claims to two waves' threads
    base = [(0, 5), (1, 5), (3, 5), (1, 8), (2, 8)]
    for arr in itertools.permutations(base):
        for split in itertools.product((0, 63, 64), repeat=len(base)):
            a = [(g, k, t) for (g, k), t in zip(arr, split)]
            P, sent, _, _ = p_per_wave(4, a, 128)
            assert P == 1 == p_per_column(4, a) and 1 <= sent <= 5


def test_the_sink_as_the_only_shared_column():
    # search 1 settled nothing (0 columns) and ends where search 0 ends; search 2 is on its own
    sets, sinks = [{10, 11, 12}, {12}, {20, 21}], [12, 12, 21]
    rng = random.Random(1)
    for how in ("kernel", "one", "random"):
        claims = deal(rng, sets, sinks, 1024, how)
        for arr in itertools.permutations(claims):
            P, sent, other, _ = p_per_wave(2, list(arr), 1024)
            assert P == 1 and sent == 1
            # search 0's claim of column 12 arrived second: ITS thread holds the flag, and the flag names search 1
            if arr.index(next(c for c in arr if c[0] == 0 and c[1] == 12)) > arr.index(next(c for c in arr if c[0] == 1)):
                assert other


def test_words_of_an_earlier_batch_flag_nobody():
    claim = {}
    arr = [(g, k, g) for g in range(4) for k in range(10)]         # batch 8: four searches over the same ten columns
    assert p_per_wave(8, arr, 64, claim)[0] == 1
    # batch 9 over the words batch 8 left, one search per column: no flag, nobody writes P
    P, sent, _, nflags = p_per_wave(9, [(0, 0, 0), (1, 1, 70), (2, 2, 5)], 128, claim)
    assert (P, sent, nflags) == (NO_CONFLICT, 0, 0)
    # ... and a word of batch 8 with a LOWER workgroup field than the arrival's flags nobody either
    claim = {3: (8 << 8) | 255}
    assert p_per_wave(9, [(4, 3, 0)], 64, claim)[:2] == (NO_CONFLICT, 0) and claim[3] == (9 << 8) | (255 - 4)
