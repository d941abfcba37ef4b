"""cyto_placeholders / place_holders_device without a device: the argument checks come before HIP is touched, a request for
no synthetic cell is answered on the host, and an unsupported dtype is refused in Python.  Also pinned here, against the
installed numpy: the argument the device path rests on -- the host loop of sample_single_cells consumes exactly the stream of
np.random.randint(0, n, size=(short, G)), and none of it when n == 1."""
import ctypes

import numpy as np
import pytest

BAD, OK = 1, 0            # CYTO_ERR_BAD_ARG, CYTO_OK
I64, U16, F64 = 5, 2, 1   # CYTO_DTYPE_*


def _call(G=4, n=3, own=True, ld_own=3, dtype=I64, short=2, out=True, ldo=2, key=True, pos=624, words=True, rbuf=0):
    from cytospace_amd import _lib
    L = _lib.lib()
    a = np.arange(12, dtype=np.int64).reshape(4, 3)
    o = np.full((4, 2), -1.0)
    k = np.arange(624, dtype=np.uint32)
    p = ctypes.c_int32(pos or 0)
    w = ctypes.c_int64(-7)
    st = L.cyto_placeholders(G, n, a.ctypes.data if own else None, ld_own, dtype, short, o.ctypes.data if out else None, ldo,
                             k.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if key else None, ctypes.byref(p) if pos is not None else None,
                             ctypes.byref(w) if words else None, rbuf, 0)
    return st, o, k, p.value, w.value


@pytest.mark.parametrize("bad", [dict(G=0), dict(G=-1), dict(n=0), dict(n=-3), dict(short=-1), dict(own=False), dict(out=False),
                                 dict(key=False), dict(pos=None), dict(ld_own=2), dict(ldo=1), dict(dtype=0), dict(dtype=3),
                                 dict(dtype=4), dict(dtype=6), dict(dtype=-1), dict(pos=-1), dict(pos=625), dict(rbuf=-1)],
                         ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_arguments_are_refused_without_a_device(bad):
    st, o, k, _, _ = _call(**bad)
    assert st == BAD
    assert np.all(o == -1.0) and np.array_equal(k, np.arange(624, dtype=np.uint32))


@pytest.mark.parametrize("pos", [0, 17, 624])
def test_no_synthetic_cell_is_ok_and_leaves_the_state(pos):
    st, o, k, p, w = _call(short=0, ldo=0, pos=pos)
    assert st == OK and p == pos and w == 0
    assert np.all(o == -1.0) and np.array_equal(k, np.arange(624, dtype=np.uint32))
    st, _, _, _, _ = _call(short=0, ldo=0, words=False)
    assert st == OK


def test_a_bad_argument_wins_over_the_empty_request():
    assert _call(short=0, ldo=0, dtype=4)[0] == BAD
    assert _call(short=0, ldo=0, pos=700)[0] == BAD


def test_place_holders_device_refuses_other_dtypes():
    from cytospace_amd.common import place_holders_device
    np.random.seed(3)
    before = np.random.get_state()
    for own in (np.array([[1, 2], [3, "x"]], dtype=object), np.ones((2, 2), np.uint64), np.ones((2, 2), bool),
                np.ones((2, 2), np.float16), np.ones((2, 2), np.complex128)):
        with pytest.raises(TypeError):
            place_holders_device(own, 3)
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_place_holders_device_empty_requests_need_no_device():
    from cytospace_amd.common import place_holders_device
    np.random.seed(4)
    np.random.standard_normal()
    before = np.random.get_state()
    out, words = place_holders_device(np.ones((5, 3), np.int64), 0, return_words=True)
    assert out.shape == (5, 0) and out.dtype == np.float64 and words == 0
    assert place_holders_device(np.ones((0, 3)), 4).shape == (0, 4)
    with pytest.raises(ValueError):
        place_holders_device(np.ones((5, 0)), 4)
    with pytest.raises(ValueError):
        place_holders_device(np.ones((5, 3)), -1)
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 100, 257])
def test_the_host_loop_is_one_randint_stream(n):
    # the reference's loop, one np.random.choice per (cell, gene), against ONE randint call of shape (short, G)
    from cytospace_amd.cytospace import _place_holders_host
    G, short = 50, 7
    own = np.random.default_rng(n).integers(0, 1000, (G, n))
    np.random.seed(n)
    np.random.randint(0, 2**32, 100, dtype=np.uint32)
    start = np.random.get_state()
    fake = _place_holders_host(own, short)
    after_loop = np.random.get_state()
    np.random.set_state(start)
    idx = np.random.randint(0, n, size=(short, G))
    after_randint = np.random.get_state()
    assert np.array_equal(fake, own[np.arange(G)[:, None], idx.T].astype(np.float64))
    assert np.array_equal(after_loop[1], after_randint[1]) and after_loop[2:] == after_randint[2:]
    if n == 1:
        assert np.array_equal(start[1], after_loop[1]) and start[2:] == after_loop[2:]
