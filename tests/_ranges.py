"""The instance pool of test_lap_ranges_*.py: float32 cost matrices far from 1 -- scaled by powers of two, below the normal range,
with -0.0, and with hundreds of binades inside one matrix.  Seeded, numpy only, nothing read from disk.

Every other LAP test draws its costs from a few binades around 1.  The solvers are documented for any finite float32 costs
(include/cytohip.h), and several of their parts depend on where in the float range the costs lie: the order keys (-0.0 sorts below
+0.0 as a key and equals it as a float), the eps schedule (built from an exponent FIELD, 0 for a subnormal gap), epsmin = vmax * 2^-23,
the absolute constants 1e-3f / 1e30f of the row-cache builders, the float64 certificate and the narrowing of the float64 warm start.

Two zones:

  exact zone   scaled(base(kind, n), k): multiplying a float32 matrix by 2^k is exact while nothing under- or overflows, and every
               add, subtract, compare and `* 2^-23` of the solvers commutes with it.  So beside the oracle of the scaled matrix there is a
               second reference that costs nothing: the scaled solve returns the base solve's indices, its duals times 2^k bit for bit and
               the same semantic counters (the wide restatement's gap_exp, an exponent field, moves by k unless it is 0, the field of a
               zero gap).  scaled() asserts the image exact and finite (one instance is not: INEXACT).
  edge classes negzero     kind 5 (integers 0 ... 9) with half of the zeros made -0.0: the values of the base, other bits
               subgrid     m * 2^-149 with integer m < 2^20: every value and every difference subnormal or tiny, and exact
               sub126      kind 1 * 2^-126, sub130: kind 1 * 2^-130 -- float32 images that are subnormal and inexact
               binades_pos 2^U(-100, 100), binades_signed: +-2^U(-60, 60) -- hundreds of binades inside one matrix
               top         kind 1 * 2^119 at n = 65 alone: the largest scale the bound below admits

No instance can overflow: _admit() asserts 2 * n * max|c| < 2^127 for every matrix of the pool (a dual is a sum of at most 2 n costs in
magnitude), and test_lap_ranges_cpu.py asserts that the oracles' own duals stay below 2^126 on every instance, on a machine
without a GPU, before a kernel sees one.  Costs near FLT_MAX, where c - v can overflow, are outside the contract (include/cytohip.h)
and outside this pool.

Sizes: 5; 65 = KC + 2 (a row cache misses columns); 300 and 1000 (the LDS-resident kernels); 2100 (the n >= 2048 rules: whole-chip first
rounds, sixteen searches at once) -- the last with kinds 1 and 2 at k = 0, +-100 and with subgrid only.  Kind 3 (every row four times)
needs n >= 8.

names() -> every instance; batch_group(n) -> the eight problems of the batch test; cost(name) -> its matrix; oracle(name, chain) -> jv_oracle / jv_oracle_wide of that matrix, solved once;
parts(name) -> (class or kind, n, k); base_of(name) -> the k = 0 instance of an exact-zone one (negzero: the kind-5 base), else None.
"""
import numpy as np

from oracle.jv import jv_oracle, jv_oracle_wide
from test_lap_batch_gpu import _make

KINDS = (1, 2, 3, 5, 8)
SCALES = (-100, -40, 40, 100)
SIZES = (5, 65, 300, 1000, 2100)
EDGES = ("negzero", "subgrid", "sub126", "sub130", "binades_pos", "binades_signed", "top")
_TAG = {c: 100 + k for k, c in enumerate(EDGES)}
_COSTS, _ORACLE = {}, {}
# the ONE scaled instance whose image is not exact: kind 1 at n = 2100 holds the value 6.8e-9 < 2^-26 (row 1731, column 1706), which loses
# two bits at 2^-127.  It stays in the pool -- the kernels against the oracle of that matrix, like sub130 -- and has no base to equal
INEXACT = ("kind1-2100-x2^-100",)


def base(kind, n):
    assert kind in KINDS
    return _make(kind, n, 0)


def _admit(c):
    n = len(c)
    assert c.dtype == np.float32 and c.shape == (n, n) and np.isfinite(c).all()
    assert 2.0 * n * float(np.abs(c).max()) < 2.0 ** 127
    return np.ascontiguousarray(c)


def scaled(c, k, exact=True):
    """c * 2^k in float32, asserted exact, finite and inside the bound."""
    c64 = c.astype(np.float64) * 2.0 ** k
    out = c64.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), c64) == exact, "the scaled image is not exact"
    return _admit(out)


def negzero(n):
    c = base(5, n).copy()
    rng = np.random.default_rng([_TAG["negzero"], n])
    c[(c == 0) & (rng.random((n, n)) < 0.5)] = np.float32(-0.0)
    assert np.array_equal(c, base(5, n))                            # (equal as floats: -0.0 == 0.0)
    assert n < 65 or (np.signbit(c).any() and ((c == 0) & ~np.signbit(c)).any())
    return _admit(c)


def subgrid(n):
    m = np.random.default_rng([_TAG["subgrid"], n]).integers(0, 1 << 20, (n, n))
    c = (m.astype(np.float64) * 2.0 ** -149).astype(np.float32)
    assert np.array_equal(c.astype(np.float64) * 2.0 ** 149, m)
    return _admit(c)


def sub126(n):
    return _admit((base(1, n).astype(np.float64) * 2.0 ** -126).astype(np.float32))


def sub130(n):
    return _admit((base(1, n).astype(np.float64) * 2.0 ** -130).astype(np.float32))


def binades_pos(n):
    return _admit((2.0 ** np.random.default_rng([_TAG["binades_pos"], n]).uniform(-100, 100, (n, n))).astype(np.float32))


def binades_signed(n):
    rng = np.random.default_rng([_TAG["binades_signed"], n])
    return _admit((rng.choice([-1.0, 1.0], (n, n)) * 2.0 ** rng.uniform(-60, 60, (n, n))).astype(np.float32))


def top(n):
    assert n == 65                                                  # 2 * 65 * 2^119 < 2^127
    return scaled(base(1, n), 119)


_EDGE_FN = dict(negzero=negzero, subgrid=subgrid, sub126=sub126, sub130=sub130, binades_pos=binades_pos,
                binades_signed=binades_signed, top=top)


def name(what, n, k=0):
    if what in EDGES:
        return f"{what}-{n}"
    return f"kind{what}-{n}" + (f"-x2^{k}" if k else "")


def parts(nm):
    f = nm.split("-", 2)
    what = int(f[0][4:]) if f[0].startswith("kind") else f[0]
    return what, int(f[1]), (int(f[2][3:]) if len(f) > 2 else 0)


def edge_sizes(cls):
    return (65,) if cls == "top" else SIZES if cls == "subgrid" else SIZES[:-1]


def names():
    out = []
    for n in SIZES:
        for kind in KINDS:
            if (kind == 3 and n < 8) or (n == 2100 and kind not in (1, 2)):
                continue
            out.append(name(kind, n))
            out += [name(kind, n, k) for k in SCALES if n < 2100 or abs(k) == 100]
        out += [name(cls, n) for cls in EDGES if n in edge_sizes(cls)]
    return out


def batch_group(n):
    """Eight same-size problems from eight corners of the range, for ONE batched call (n = 96 is the size test_lap_batch_gpu.py uses
    for group logic; these instances exist at any n)."""
    return [name(1, n, -100), name(1, n), name(1, n, 100), name(2, n, -100), name(2, n, 100), name("subgrid", n),
            name("negzero", n), name("binades_signed", n)]


def is_exact_zone(nm):
    return isinstance(parts(nm)[0], int) and nm not in INEXACT


def base_of(nm):
    what, n, k = parts(nm)
    if isinstance(what, int):
        return name(what, n) if k and nm not in INEXACT else None
    return name(5, n) if what == "negzero" else None


def cost(nm):
    if nm not in _COSTS:
        what, n, k = parts(nm)
        if isinstance(what, int):
            c = _admit(base(what, n))
            _COSTS[nm] = scaled(c, k, nm not in INEXACT) if k else c
        else:
            _COSTS[nm] = _EDGE_FN[what](n)
    return _COSTS[nm]


def oracle(nm, chain):
    key = (nm, bool(chain))
    if key not in _ORACLE:
        _ORACLE[key] = jv_oracle(cost(nm), np.float32) if chain else jv_oracle_wide(cost(nm), np.float32)
    return _ORACLE[key]
