"""downsample_device (C ABI: cyto_downsample) against the host `downsample` on the GPU: the same DataFrame and the same
numpy global state afterwards, draw for draw; the raw generator (cyto_mt19937_fill) against numpy's words; the errors."""
import os

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] and a[4] == b[4]


def _check(values, target, seed, dtype=np.int64, index=None, columns=None):
    from cytospace_amd.common import downsample, downsample_device
    df = pd.DataFrame(values, index=index, columns=columns)
    np.random.seed(seed)
    np.random.standard_normal()                       # a cached gaussian must survive the call
    host = downsample(df, target)
    after_host = np.random.get_state()
    np.random.seed(seed)
    np.random.standard_normal()
    dev = downsample_device(df, target, dtype=dtype)
    after_dev = np.random.get_state()
    assert all(dev.dtypes == np.dtype(dtype))
    assert np.array_equal(dev.to_numpy(), host.to_numpy())
    assert list(dev.index) == list(host.index) and list(dev.columns) == list(host.columns)
    assert _same_state(after_dev, after_host)
    return dev


def test_gv13():
    d = np.load(os.path.join(ROOT, "tests", "golden", "gv13_downsample.npz"))
    np.random.seed(int(d["seed"]))
    from cytospace_amd.common import downsample_device
    df = pd.DataFrame(d["counts"], index=[f"GENE_{i}" for i in range(40)], columns=[f"CELL_{i}" for i in range(9)])
    out = downsample_device(df, int(d["target"]))
    assert np.array_equal(out.to_numpy(), d["out"])
    _check(d["counts"], int(d["target"]), int(d["seed"]), index=df.index, columns=df.columns)


@pytest.mark.parametrize("G,C,target,seed", [(1, 1, 3, 0), (1, 17, 5, 1), (300, 1, 40, 2), (257, 65, 100, 3), (3000, 40, 1500, 4),
                                             (4100, 30, 700, 5), (90, 300, 1, 6), (50, 50, 2, 7)])
def test_random_shapes(G, C, target, seed):
    rng = np.random.default_rng(seed)
    x = rng.poisson(rng.lognormal(0, 1.5, (G, 1)) * 0.5, (G, C)).astype(np.int64)
    x[:, ::3] //= 4
    _check(x, target, seed + 10)


def test_all_cells_under_the_target_take_no_words():
    x = np.random.default_rng(1).integers(0, 3, (40, 12))
    _check(x, 10**6, 3)


def test_one_nonzero_gene():
    x = np.zeros((500, 6), np.int64)
    x[321] = [5000, 10, 3, 7000, 1, 200]
    _check(x, 50, 8)


@pytest.mark.parametrize("k", [2, 7, 16, 20])
def test_totals_at_the_mask_edges(k):
    # cell totals 2^k - 1, 2^k, 2^k + 1 (the mask changes between the first two); few genes keep np.repeat small
    for T in (2**k - 1, 2**k, 2**k + 1):
        x = np.zeros((3, 2), np.int64)
        x[0] = T // 2
        x[2] = T - T // 2
        _check(x, 3, k)


@pytest.mark.parametrize("T", [2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1, 2**32])
def test_totals_near_2_31_and_2_32(T):
    # the host's np.repeat would need T * 8 bytes here: its draws are restated as what np.random.choice does with
    # replacement, randint(0, T, target), mapped to genes by the cumulative counts
    from cytospace_amd.common import downsample_device
    x = np.zeros((3, 2), np.int64)
    x[0] = T // 3
    x[2] = T - T // 3
    np.random.seed(T % 1000)
    want = np.zeros_like(x)
    for c in range(2):
        r = np.random.randint(0, T, 700)
        want[:, c] = np.bincount(np.searchsorted(np.cumsum(x[:, c]), r, side="right"), minlength=3)
    after = np.random.get_state()
    np.random.seed(T % 1000)
    got = downsample_device(pd.DataFrame(x), 700)
    assert np.array_equal(got.to_numpy(), want) and _same_state(after, np.random.get_state())


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32, np.int64, np.int16, np.uint32, np.bool_])
def test_input_dtypes(dtype):
    x = np.random.default_rng(3).integers(0, 2 if dtype == np.bool_ else 120, (70, 30)).astype(dtype)
    _check(x, 1 if dtype == np.bool_ else 400, 21)


def test_uint16_output():
    x = np.random.default_rng(4).integers(0, 200, (300, 40))
    _check(x, 1000, 5, dtype=np.uint16)


@pytest.mark.parametrize("seed", [0, 1, 2**31, 2**32 - 1])
def test_seeds(seed):
    x = np.random.default_rng(seed % 97).integers(0, 30, (200, 25))
    _check(x, 300, seed)


def test_many_blocks_ending_on_pos_624():
    # totals 2^10 (every word accepted): 3 cells x 590 draws use the rest of the key after pos 102 and two more keys exactly
    from cytospace_amd.common import downsample_device
    x = np.full((2, 3), 512, np.int64)
    np.random.seed(9)
    np.random.randint(0, 2**32, 102, dtype=np.uint32)
    st = np.random.get_state()
    dev, words = downsample_device(pd.DataFrame(x), 590, return_words=True)
    after = np.random.get_state()
    np.random.set_state(st)
    from cytospace_amd.common import downsample
    host = downsample(pd.DataFrame(x), 590)
    assert words == 1770 and after[2] == 624 and _same_state(after, np.random.get_state())
    assert np.array_equal(dev.to_numpy(), host.to_numpy())


def test_stream_crossing_blocks_of_cells():
    # blocks of 3 cells (CYTO_DS_RBUF_BYTES, read once per process: a fresh interpreter): 17 blocks, stage 1 of each one
    # overlapping stage 2 of the one before, the MT19937 state handed from block to block
    import subprocess
    import sys
    code = ("import numpy as np, pandas as pd\n"
            "from cytospace_amd.common import downsample, downsample_device\n"
            "x = pd.DataFrame(np.random.default_rng(8).integers(0, 40, (300, 50)))\n"
            "np.random.seed(4); h = downsample(x, 300); sh = np.random.get_state()\n"
            "np.random.seed(4); d = downsample_device(x, 300); sd = np.random.get_state()\n"
            "assert np.array_equal(h.to_numpy(), d.to_numpy())\n"
            "assert np.array_equal(sh[1], sd[1]) and sh[2] == sd[2]\n"
            "print('ok')\n")
    env = dict(os.environ, CYTO_DS_RBUF_BYTES=str(3 * 300 * 4), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-3000:]


def test_large_instance():
    rng = np.random.default_rng(20)
    G, C = 2000, 20000
    rate = rng.lognormal(0, 1.2, G)
    rate *= 1500.0 / rate.sum()
    x = rng.poisson(rate[:, None] * rng.lognormal(0, 0.5, (1, C))).astype(np.int64)
    _check(x, 1000, 33)


@pytest.mark.parametrize("pos", [1, 300, 623, 624])
def test_raw_fill_equals_numpy_words(pos):
    from cytospace_amd.common import mt19937_fill
    np.random.seed(77)
    np.random.randint(0, 2**32, 624 + pos if pos < 624 else 624, dtype=np.uint32)
    st = np.random.get_state()
    assert st[2] == pos
    got = mt19937_fill(5000)
    after = np.random.get_state()
    np.random.set_state(st)
    want = np.random.randint(0, 2**32, 5000, dtype=np.uint32)
    assert np.array_equal(got, want) and _same_state(after, np.random.get_state())


def test_errors_before_any_draw():
    from cytospace_amd.common import downsample, downsample_device
    np.random.seed(1)
    st = np.random.get_state()
    neg = pd.DataFrame(np.array([[5, 1], [-1, 0], [9, 1]]))
    with pytest.raises(ValueError):
        downsample_device(neg, 3)                                   # the first cell is downsampled and holds a negative count
    with pytest.raises(ValueError):
        downsample(neg, 3)
    np.random.set_state(st)
    with pytest.raises(TypeError):
        downsample_device(pd.DataFrame(np.ones((3, 2))), 1)
    with pytest.raises(TypeError):
        downsample(pd.DataFrame(np.ones((3, 2)) * 3), 1)
    big = pd.DataFrame(np.array([[2**32], [1]], np.int64))         # total 2^32 + 1
    with pytest.raises(ValueError):
        downsample_device(big, 5)
    assert _same_state(st, np.random.get_state())


def test_negative_count_in_a_kept_cell_is_copied():
    x = np.array([[5, 1], [-1, 0], [9, 1]])
    _check(x, 20, 2)
    x2 = np.array([[50, -3], [60, 2], [1, 1]])
    _check(x2, 30, 2)


def test_target_zero():
    x = np.random.default_rng(2).integers(0, 4, (10, 6))
    x[:, 2] = 0
    _check(x, 0, 5)


def test_two_runs_are_identical():
    from cytospace_amd.common import downsample_device
    x = pd.DataFrame(np.random.default_rng(6).integers(0, 50, (400, 60)))
    np.random.seed(3)
    a = downsample_device(x, 500)
    np.random.seed(3)
    b = downsample_device(x, 500)
    assert a.equals(b)
