"""Value sets of the fractional text writers' tests (test_text_fractions_cpu.py, test_text_fractions_gpu.py), and the libraries' own
text for them: scipy.io.mmwrite's entry lines and DataFrame.to_csv's fields, taken at run time."""
import io

import numpy as np
import pandas as pd

CODES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint16): 2, np.dtype(np.uint8): 3, np.dtype(np.int32): 4,
         np.dtype(np.int64): 5}
FRACTIONS = 1                                  # CYTO_TEXT_FRACTIONS
BAD_ARG, UNSUPPORTED = 1, 7
UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def finite(a):
    return a[np.isfinite(a)]


def random_bits(dtype, n, seed):
    """n random bit patterns of the type, the non-finite ones dropped: every exponent is as likely as any other."""
    u = UINT[np.dtype(dtype)]
    bits = np.random.default_rng(seed).integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True)
    return finite(bits.view(dtype))


def neighbours(a):
    """a with the value below and above each element, of a's own dtype."""
    a = np.asarray(a)
    with np.errstate(over="ignore"):
        return finite(np.concatenate([np.nextafter(a, a.dtype.type(-np.inf)), a, np.nextafter(a, a.dtype.type(np.inf))]))


def edge_values(dtype):
    """Positive values where a digit routine goes wrong: every power of two of the type with its two neighbours (the uneven rounding
    intervals), every power of ten in range with its neighbours, the smallest and largest subnormal, the smallest normal, the maximum,
    k / 10^j for every digit count, and the integers around 2^24 / 2^53 where the writers' integer path ends."""
    dtype = np.dtype(dtype)
    fi = np.finfo(dtype)
    t = dtype.type
    with np.errstate(over="ignore", under="ignore"):
        two = np.ldexp(t(1), np.arange(fi.minexp - fi.nmant, fi.maxexp)).astype(dtype)
        ten = np.array([float("1e%d" % k) for k in range(-330, 310)]).astype(dtype)        # (correctly rounded: parsed, not computed)
    ten = ten[(ten > 0) & np.isfinite(ten)]
    ndig = 9 if dtype == np.float32 else 17
    rng = np.random.default_rng(11)
    frac = []
    for nd in range(1, ndig + 1):
        for j in (0, 1, 2, 3, 4, 5, 6, 7, 10, 16, 17, 20, 25, 40, 300, -1, -2, -5, -10, -15, -16, -17, -20, -30):
            for k in [10**(nd - 1), 10**nd - 1] + [int(v) for v in rng.integers(10**(nd - 1), 10**nd, 6)]:
                frac.append(float("%de%d" % (k, -j)))
    with np.errstate(over="ignore", under="ignore"):
        frac = np.array(frac).astype(dtype)
    lim = 2**(fi.nmant + 1)
    ints = np.array([lim - 2, lim - 1, lim, lim + 2, lim + 4, 2 * lim, 2 * lim + 4, 10 * lim, lim // 2 + 1, lim // 2 + 0.5, lim // 4 + 0.25, 1.0, 10.0,
                     1e15, 1e16, 1e17, 123456.0, 1234567.0, 2500.0], np.float64).astype(dtype)
    special = np.array([fi.smallest_subnormal, fi.smallest_normal, fi.max, np.nextafter(t(fi.smallest_normal), t(0))], dtype)
    form = np.array([1e-4, 1e-5, 1.5e-5, 9.999e-5, 1.234e-4, 9.99e15, 1e16, 1.5e16, 1e15, 1e-3, 0.5, 0.1, 1 / 3, 2.5, 1e22, 1e23], np.float64).astype(dtype)
    out = np.concatenate([neighbours(two), neighbours(ten), frac, neighbours(ints), special, neighbours(form)])
    return finite(out[out > 0])


def form_switch(dtype):
    """The values around the CSV layout's switch between its two forms: a float32 within 4096 ulps of 1e-4 and of 1e16, and the
    float64 neighbours of both; the first and last value of the decimal exponents -5, -4, 15, 16."""
    dtype = np.dtype(dtype)
    out = []
    for c in (1e-4, 1e16):
        if dtype == np.float32:
            b = np.array([c], np.float32).view(np.uint32)[0]
            out.append(np.arange(int(b) - 4096, int(b) + 4097, dtype=np.uint32).view(np.float32))
        else:
            b = np.array([c], np.float64).view(np.uint64)[0]
            out.append(np.arange(int(b) - 64, int(b) + 65, dtype=np.uint64).view(np.float64))
    out.append(neighbours(np.array([1e-5, 9.999999999999999e-5, 1e-4, 9.999999999999999e-4, 1e15, 9.999999999999998e15, 1e16, 9.999999999999998e16],
                                   np.float64).astype(dtype)))
    return np.concatenate(out)


def all_values(dtype, nrandom, seed=5):
    """Every set above and nrandom random bit patterns, both signs, zeros of both signs."""
    pos = np.concatenate([edge_values(dtype), form_switch(dtype), np.abs(random_bits(dtype, nrandom, seed))])
    pos = pos[pos > 0]
    return np.concatenate([pos, -pos[::3], np.array([0.0, -0.0], dtype)])


def mixed_matrix(dtype, G, C, seed, zeros=0.0):
    """G x C values of every class: all digit counts, both forms, integers inside and outside the integer window, zeros of both
    signs; `zeros`: the share of entries set to zero afterwards."""
    rng = np.random.default_rng(seed)
    pool = all_values(dtype, 2000, seed)
    x = pool[rng.integers(0, len(pool), G * C)].reshape(G, C)
    small = rng.random((G, C)) < 0.3                                     # what expression tables hold: short fractions and counts
    x[small] = np.round(rng.random(int(small.sum())) * 100, 2).astype(dtype)
    whole = rng.random((G, C)) < 0.2
    x[whole] = rng.integers(-3, 3000, int(whole.sum())).astype(dtype)
    x[rng.random((G, C)) < 0.05] = np.dtype(dtype).type(-0.0)
    if zeros:
        x[rng.random((G, C)) < zeros] = 0
    return np.ascontiguousarray(x)


def scipy_bytes(x, columns=None):
    """The file scipy.io.mmwrite writes for coo_matrix(x[:, columns])."""
    import scipy.io
    import scipy.sparse
    buf = io.BytesIO()
    scipy.io.mmwrite(buf, scipy.sparse.coo_matrix(x if columns is None else x[:, columns]))
    return buf.getvalue()


def scipy_body(values):
    """The entry lines scipy writes for the n x 1 matrix of `values` (n != 1)."""
    text = scipy_bytes(np.asarray(values).reshape(-1, 1))
    head = b"".join(text.split(b"\n", 3)[:3]) + b"\n\n\n"
    assert text.startswith(b"%%MatrixMarket matrix coordinate real general\n")
    return text[len(head):]


def pandas_fields_text(values):
    """The fields DataFrame.to_csv writes for a one-column frame of `values`, each followed by a newline."""
    return pd.DataFrame({"v": np.asarray(values)}).to_csv(index=False, header=False).encode()


def pandas_bytes(x, columns, index_labels=None, column_labels=None):
    out = pd.DataFrame(x[:, columns])
    if index_labels is not None:
        out.index = index_labels
    if column_labels is not None:
        out.columns = column_labels
    return out.to_csv().encode()
