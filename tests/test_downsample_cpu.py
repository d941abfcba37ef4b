"""CPU tests of the downsample kernel's algorithm (cytospace_amd/csrc/downsample.hip), restated in numpy: the in-place twist
in three slices of 227 / 227 / 170 words, the acceptance test 64 words at a time with the cut inside a group when a cell
ends, cells processed in blocks with the state handed from block to block.  Pinned against the installed numpy: its raw
words (np.random.randint(0, 2**32, dtype=np.uint32)), the host `downsample` and np.random.get_state() afterwards."""
import numpy as np
import pandas as pd
import pytest

N, M = 624, 397
SLICES = ((0, 227), (227, 454), (454, 624))


def temper(y):
    y = y.astype(np.uint32)
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def twist_slice(key, lo, hi):
    i = np.arange(lo, hi)
    y = (key[i] & np.uint32(0x80000000)) | (key[(i + 1) % N] & np.uint32(0x7FFFFFFF))
    new = key[(i + M) % N] ^ (y >> np.uint32(1)) ^ ((np.uint32(0) - (y & np.uint32(1))) & np.uint32(0x9908B0DF))
    key[lo:hi] = new                      # every read of the slice before any write, as in the kernel


def gen_mask(rng):
    return (1 << int(rng).bit_length()) - 1


def stream(key, pos, rngs, target):
    """ds_stream: returns (r rows, key, pos, words) for the cells with ranges rngs (T - 1)."""
    key = key.copy()
    rows = np.zeros((len(rngs), target), np.uint32)
    if not len(rngs) or target == 0:
        return rows, key, pos, 0
    d, k, used, end = 0, 0, 0, pos
    rng = int(rngs[0]); mask = gen_mask(rng)
    sl = 0 if pos >= N else -1
    done = False
    while not done:
        lo, hi = (pos, N) if sl < 0 else SLICES[sl]
        if sl >= 0:
            twist_slice(key, lo, hi)
        s = lo
        while s < hi:
            w = temper(key[s:min(s + 64, hi)]).astype(np.int64) & mask
            acc = w <= rng
            n = int(acc.sum())
            need = target - k
            if n < need:
                rows[d, k:k + n] = w[acc]
                k += n
                s += 64
                continue
            L = int(np.flatnonzero(acc)[need - 1])
            rows[d, k:] = w[:L + 1][acc[:L + 1]]
            s += L + 1
            k = 0
            d += 1
            if d == len(rngs):
                done, end = True, s
                break
            rng = int(rngs[d]); mask = gen_mask(rng)
        used += (end if done else hi) - lo
        if not done:
            sl = 0 if sl == 2 else sl + 1
    if sl in (0, 1):
        for q in range(sl + 1, 3):
            twist_slice(key, *SLICES[q])
    return rows, key, end, used


def restated_downsample(values, target, state, block_cells=None):
    """The whole of cyto_downsample on the host: totals, copies, blocks of stage 1, stage 2 (upper-bound + histogram)."""
    key, pos = np.array(state[1], np.uint32), int(state[2])
    tot = values.sum(axis=0, dtype=np.int64)
    cells = np.flatnonzero(tot > target)
    out = values.astype(np.int64)
    per = block_cells or max(1, len(cells))
    words = 0
    for b0 in range(0, len(cells), per):
        blk = cells[b0:b0 + per]
        rows, key, pos, used = stream(key, pos, tot[blk] - 1, target)
        words += used
        for j, c in enumerate(blk):
            cum = np.cumsum(values[:, c], dtype=np.int64)
            out[:, c] = np.bincount(np.searchsorted(cum, rows[j].astype(np.int64), side="right"), minlength=len(cum))
    return out, key, pos, words


def reach(seed, pos):
    """Seed numpy's global generator and move it to `pos` (0: a freshly twisted key no word of which is used yet)."""
    np.random.seed(seed)
    if 0 < pos < 624:
        np.random.randint(0, 2**32, 624 + pos, dtype=np.uint32)
    elif pos == 0:
        st = np.random.get_state()
        key = np.array(st[1], np.uint32)
        for sl in SLICES:
            twist_slice(key, *sl)
        np.random.set_state((st[0], key, 0, st[3], st[4]))


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] and a[4] == b[4]


@pytest.mark.parametrize("pos", [624, 0, 1, 226, 227, 300, 453, 454, 600, 623])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 170, 227, 397, 624, 1000, 2500])
def test_restated_stream_equals_numpy_words(pos, n):
    reach(5, pos)
    st = np.random.get_state()
    assert st[2] == pos
    rows, key, p, used = stream(np.array(st[1], np.uint32), st[2], [2**32 - 1], n)
    want = np.random.randint(0, 2**32, n, dtype=np.uint32)
    after = np.random.get_state()
    assert np.array_equal(rows[0], want) and used == n
    assert np.array_equal(key, after[1]) and p == after[2]


def _counts(rng, G, C, lo=0, hi=60):
    return rng.integers(lo, hi, (G, C)).astype(np.int64)


@pytest.mark.parametrize("seed,G,C,target,block", [(0, 300, 60, 500, None), (1, 50, 40, 7, 3), (2, 1, 9, 3, None),
                                                    (3, 120, 1, 40, None), (4, 40, 30, 1, 4), (5, 200, 25, 900, 2)])
def test_restated_downsample_equals_host_downsample(seed, G, C, target, block):
    from cytospace_amd.common import downsample
    rng = np.random.default_rng(seed)
    values = _counts(rng, G, C)
    values[:, ::5] //= 8                                           # a mix of kept and downsampled cells
    np.random.seed(seed + 100)
    state = np.random.get_state()
    out, key, pos, words = restated_downsample(values, target, state, block)
    df = pd.DataFrame(values)
    host = downsample(df, target)
    after = np.random.get_state()
    assert np.array_equal(out, host.to_numpy())
    assert np.array_equal(key, after[1]) and pos == after[2]


def test_ends_on_pos_624():
    # pick the target so that the last accepted word is key[623]: consume exactly to the end of a key
    from cytospace_amd.common import downsample
    values = np.zeros((2, 3), np.int64)
    values[0] = 512                                              # T = 2^10 per cell: mask == T - 1, every word is accepted
    values[1] = 512
    np.random.seed(9)
    np.random.randint(0, 2**32, 102, dtype=np.uint32)            # pos = 102
    state = np.random.get_state()
    target = (624 - 102 + 624 * 2) // 3                           # 3 cells x target words == the rest of this key + two keys
    assert (624 - 102 + 624 * 2) % 3 == 0 and target < 1024
    out, key, pos, words = restated_downsample(values, target, state, 2)
    host = downsample(pd.DataFrame(values), target)
    after = np.random.get_state()
    assert pos == 624 == after[2] and words == 3 * target
    assert np.array_equal(key, after[1]) and np.array_equal(out, host.to_numpy())


@pytest.mark.parametrize("k", [1, 2, 5, 13, 20])
def test_totals_at_mask_edges(k):
    from cytospace_amd.common import downsample
    for T in (2**k, 2**k + 1, 2**k - 1):
        if T < 3:
            continue
        values = np.array([[T // 3, T // 3], [T - 2 * (T // 3), T - 2 * (T // 3)], [0, 0]], np.int64)
        target = 2
        np.random.seed(k)
        state = np.random.get_state()
        out, key, pos, _ = restated_downsample(values, target, state, 1)
        host = downsample(pd.DataFrame(values), target)
        after = np.random.get_state()
        assert np.array_equal(out, host.to_numpy()), T
        assert np.array_equal(key, after[1]) and pos == after[2], T


def test_target_zero_consumes_no_words():
    from cytospace_amd.common import downsample
    values = np.array([[3, 0, 1], [2, 0, 0]], np.int64)
    np.random.seed(4)
    state = np.random.get_state()
    out, key, pos, words = restated_downsample(values, 0, state)
    host = downsample(pd.DataFrame(values), 0)
    assert words == 0 and np.array_equal(out, np.zeros_like(values)) and np.array_equal(host.to_numpy(), out)
    assert _state_equal(state, np.random.get_state())


def test_gv13_restated():
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gv13_downsample.npz"))
    np.random.seed(int(d["seed"]))
    out, _, _, _ = restated_downsample(d["counts"], int(d["target"]), np.random.get_state(), 2)
    assert np.array_equal(out, d["out"])
