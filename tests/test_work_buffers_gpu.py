"""Work buffers: no result may depend on what a block of the device cache (core.hip: cache_alloc, DevBuf) or a plain large buffer
(cyto::Mem) held when the library took it.  Neither source initialises what it hands out: a fresh hipMalloc block usually arrives
zeroed, a reused one holds a well-formed state of the previous solve, so a word that a kernel reads before anyone wrote it -- a tag, a
counter, a list length, a barrier word, a padding lane of a 16-byte load -- passes every other module of the suite.

The poison hook (cyto_cache_poison, include/cytohip.h) fills every block on its way out with one byte.  Every case here runs its call
EIGHT times: for each of the four patterns

    0x00   zero                                   the control: the harness agrees with the reference
    0xFF   -1 as int32, NaN as a float            code that relies on an accidental "unassigned" sentinel
    0x7F   2139062143 as int32, 3.39e38 float32
    0x80   -2139062144 as int32, -1.18e-38 float32

once after cyto_trim_device_cache (every block fresh and filled) and once more without trimming (every block reused and refilled),
and asserts
  1. cyto_cache_poison_fills() advanced during the call (otherwise the case is vacuous);
  2. the result against the call's own reference, never the library's run with the poison off: LAPs against the CPU oracle
     (oracle/jv.py) -- rowsol, colsol, u, v and the BITS of total, the status (a non-zero one raises); cost-build outputs against the
     float64 references of oracle/cost.py and oracle/precision.py with the tolerances of tests/test_cost_precision_gpu.py; the other
     device paths against the CPU models of their own GPU tests;
  3. every output of the eight runs is bit-identical to the first run's.

The bits of total: the kernels add the assigned costs in a tree, the oracle one after the other.  The LAP instances here hold float32
values (the float64 solves too, as tests/test_lap_gpu.py::test_uniform has them), a few thousand of them within a few binades: every
partial sum of either order is exact in float64, so the two totals are the same number.

Cases that need a once-per-process knob (the embedded searches, the column reduction's lists) run in one child interpreter each,
which switches the poison on itself.  The batch entry point of the C ABI takes no row maps: row maps in a batch go through
cyto_ctx_assign_chunks (slot counts that repeat spots), as tests/test_lap_batch_gpu.py (f) has them.
"""
import ctypes
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import _layouts as LY
from cytospace_amd import _lib
from cytospace_amd import common as gcommon
from cytospace_amd import cytospace as gcyto
from cytospace_amd.lap import lap_solve, lap_solve_batch, lap_solve_rows
from oracle import cost as ocost
from oracle import precision as P
from oracle.jv import jv_oracle, jv_oracle_wide
from test_cost_precision_gpu import METRICS, SENTINEL, TOL, TRANSFORMS, _cost_metric, _transform, _up

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = (0x00, 0xFF, 0x7F, 0x80)
LAP_KEYS = ("rowsol", "colsol", "u", "v")


@pytest.fixture(autouse=True)
def _poison_off_afterwards():
    """Whatever a case did or however it failed: the poison is off and the cache empty for whoever runs next."""
    try:
        yield
    finally:
        _lib.lib().cyto_cache_poison(-1)
        _lib.lib().cyto_trim_device_cache(0)


# ---- the harness --------------------------------------------------------------------------------------------------------------

def _bits(x):
    """An output as something that compares bit for bit (NaN equals itself, -0.0 differs from +0.0)."""
    if isinstance(x, dict):
        return tuple((k, _bits(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return tuple(_bits(y) for y in x)
    if isinstance(x, pd.DataFrame):
        return (tuple(map(str, x.index)), tuple(map(str, x.columns)), tuple(str(t) for t in x.dtypes), _bits(x.to_numpy()))
    if isinstance(x, np.ndarray):
        if x.dtype == object:
            return tuple(_bits(y) for y in x.ravel().tolist())
        return (x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (float, np.floating)):
        return struct.pack("<d", float(x))
    if isinstance(x, (int, np.integer, str, bytes, bool, type(None))):
        return x
    raise TypeError(type(x))


def _eight(call, check=None):
    """call() under every pattern, on fresh blocks and on reused ones; check(out, tag) against the reference; the eight outputs
    bit-identical.  Returns the last output."""
    outs, tags, out = [], [], None
    for byte in PATTERNS:
        _lib.cache_poison(byte)
        for blocks in ("fresh", "reused"):
            if blocks == "fresh":
                _lib.trim_device_cache()
            tag = f"pattern 0x{byte:02X}, {blocks} blocks"
            f0, b0 = _lib.cache_poison_fills(), _lib.cache_poison_bytes()
            out = call()
            fills, nbytes = _lib.cache_poison_fills() - f0, _lib.cache_poison_bytes() - b0
            assert fills > 0 and nbytes > 0, f"{tag}: the call took no block from the cache ({fills} fills): the case is vacuous"
            if check is not None:
                check(out, tag)
            outs.append(_bits(out))
            tags.append(tag)
    _lib.cache_poison(None)
    for o, tag in zip(outs[1:], tags[1:]):
        assert o == outs[0], f"{tag}: the output differs from the one under {tags[0]}"
    return out


def _same_total(a, b):
    return struct.pack("<d", float(a)) == struct.pack("<d", float(b))


def _lap_out(g):
    return dict(rowsol=g["rowsol"], colsol=g["colsol"], u=g["u"], v=g["v"], total=g["total"], status=0)     # (a status raises)


def _lap_check(o, cast=None):
    def check(out, tag):
        for k in LAP_KEYS:
            want = o[k] if cast is None or k in ("rowsol", "colsol") else o[k].astype(cast)
            assert np.array_equal(out[k], want), f"{tag}: {k} differs from the oracle in {(out[k] != want).sum()} of {len(want)} entries"
        assert _same_total(out["total"], o["total"]), f"{tag}: total {out['total']!r}, the oracle's {o['total']!r}"
    return check


_ORACLE = {}


def _oracle(name, make):
    if name not in _ORACLE:
        _ORACLE[name] = make()
    return _ORACLE[name]


def _uniform(n):
    return np.random.default_rng(n).random((n, n)).astype(np.float32)            # (tests/test_lap_gpu.py::test_uniform)


def _wide_case(name, c, opts=None, rounds=0, solve=None):
    o = _oracle(("wide", name, rounds), lambda: jv_oracle_wide(c, np.float32, max_rounds=-1 if rounds == 0 else max(rounds, 0)))
    solve = solve or (lambda: lap_solve(c, np.float32, return_info=True, opts=dict(mode=2, **opts) if opts else None))

    def call():
        g = solve()
        assert g["info"].wide == 1
        return _lap_out(g)
    return _eight(call, _lap_check(o))


# ---- the hook itself ------------------------------------------------------------------------------------------------------------

PEEK_SIZES = (1, 257, (3 << 20) + 1)


def test_cache_peek_reads_the_pattern_back_fresh_and_after_a_solve():
    c = _uniform(1000)
    for byte in PATTERNS[1:] + PATTERNS[:1]:
        _lib.cache_poison(byte)
        _lib.trim_device_cache()
        for when in ("fresh", "after a solve", "again"):
            if when == "after a solve":
                lap_solve(c, np.float32)              # returns blocks of many sizes, the 256-byte ones among them, with its state in them
            for size in PEEK_SIZES:
                f0, b0 = _lib.cache_poison_fills(), _lib.cache_poison_bytes()
                got = _lib.cache_peek(size)
                assert got.shape == (size,) and (got == byte).all(), (hex(byte), when, size, np.flatnonzero(got != byte)[:8])
                assert _lib.cache_poison_fills() == f0 + 1 and _lib.cache_poison_bytes() - b0 >= size       # (the whole rounded block)
    # off: nothing is filled, by a peek or by a solve
    _lib.cache_poison(None)
    f0, b0 = _lib.cache_poison_fills(), _lib.cache_poison_bytes()
    lap_solve(c, np.float32)
    for size in PEEK_SIZES:
        _lib.cache_peek(size)
    assert (_lib.cache_poison_fills(), _lib.cache_poison_bytes()) == (f0, b0)
    L = _lib.lib()
    assert L.cyto_cache_poison(256) == 1 and L.cyto_cache_poison(-2) == 1 and L.cyto_cache_poison(-1) == 0       # CYTO_ERR_BAD_ARG
    room = np.zeros(16, np.uint8)
    assert L.cyto_cache_peek(0, room.ctypes.data, 0) == 1 and L.cyto_cache_peek(16, None, 0) == 1


# ---- the wide solver, float32 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 65, 300, 1000, 2500])
def test_wide_uniform(n):
    # 2500: several searches at once by default (from 2 048 rows on)
    _wide_case(f"uniform{n}", _uniform(n))


def test_wide_integer_ties_unscaled():
    c = np.random.default_rng(300).integers(0, 10, (300, 300)).astype(np.float32)
    _wide_case("ties300", c)


def test_wide_duplicated_rows_through_the_row_map():
    # runs of 100 identical rows (tests/test_lap_gpu.py::test_wide_one_edge_searches_on_the_whole_chip (d)): the one-edge searches of
    # the whole chip, their claim words and lists
    rng = np.random.default_rng(91)
    rows = -(rng.random((12, 1200)) ** 3).astype(np.float32)
    rowmap = np.repeat(np.arange(12), 100).astype(np.int32)
    g = _wide_case("long_runs", rows[rowmap], solve=lambda: lap_solve_rows(rows, rowmap, return_info=True, opts=dict(mode=2)))
    assert np.array_equal(np.bincount(rowmap[g["colsol"]], minlength=12), np.full(12, 100))


@pytest.mark.parametrize("opts", [dict(wide_par=5), dict(wide_rebuild=1), dict(wide_wipe=1), dict(wide_rounds=3), dict(cache_waves=1),
                                  dict(cache_stream=-1)], ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_wide_options_at_1000(opts):
    _wide_case("uniform1000", _uniform(1000), opts, rounds=opts.get("wide_rounds", 0))


_CHILD = r'''
import json, sys
import numpy as np
from cytospace_amd import _lib
from cytospace_amd.lap import lap_solve
from oracle.jv import jv_oracle_wide

case = sys.argv[1]
n, opts = (700, dict(mode=2, wide_par=5)) if case == "embedded" else (2051, dict(mode=2))
c = np.random.default_rng(42).random((n, n)).astype(np.float32)
o = jv_oracle_wide(c, np.float32)
e0, s0 = _lib.wide_embedded_solves(), _lib.fused_cache_solves()
runs, fills, bad, first = 0, [], [], None
for byte in (0x00, 0xFF, 0x7F, 0x80):
    _lib.cache_poison(byte)
    for fresh in (True, False):
        if fresh:
            _lib.trim_device_cache()
        f0 = _lib.cache_poison_fills()
        g = lap_solve(c, np.float32, return_info=True, opts=opts)
        fills.append(_lib.cache_poison_fills() - f0)
        tag = "0x%02X %s" % (byte, "fresh" if fresh else "reused")
        for k in ("rowsol", "colsol", "u", "v"):
            if not np.array_equal(g[k], o[k]):
                bad.append("%s: %s differs from the oracle in %d entries" % (tag, k, int((g[k] != o[k]).sum())))
        if np.float64(g["total"]).tobytes() != np.float64(o["total"]).tobytes():
            bad.append("%s: total %r, the oracle's %r" % (tag, g["total"], o["total"]))
        bits = tuple(g[k].tobytes() for k in ("rowsol", "colsol", "u", "v")) + (np.float64(g["total"]).tobytes(),)
        first = first or bits
        if bits != first:
            bad.append(tag + ": differs from the first run")
        runs += 1
_lib.cache_poison(None)
print(json.dumps({"runs": runs, "fills": fills, "bad": bad, "embedded": _lib.wide_embedded_solves() - e0,
                  "fused": _lib.fused_cache_solves() - s0}))
'''


def _child(tmp_path, case, knobs):
    script = tmp_path / "work_buffers_child.py"
    script.write_text(_CHILD)
    env = {k: v for k, v in os.environ.items() if k not in ("CYTO_AUG_LDS", "CYTO_AUG_EMBED", "CYTO_CACHE_FUSED")}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, env.get("PYTHONPATH", "")])
    env.update(knobs)
    r = subprocess.run([sys.executable, str(script), case], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, out)
    assert out["runs"] == 8 and not out["bad"], out["bad"]
    assert all(f > 0 for f in out["fills"]), out["fills"]
    return out


def test_wide_embedded_searches_in_a_child(tmp_path):
    # wide_aug<.., EMB>: cache_red, the inverse index and its counts carved behind the search state (tests/test_wide_embedded_gpu.py)
    out = _child(tmp_path, "embedded", dict(CYTO_AUG_LDS="1", CYTO_AUG_EMBED="2"))
    assert out["embedded"] == 8


def test_column_reduction_lists_in_a_child(tmp_path):
    # the first row caches from the column reduction's lists (tests/test_cache_fused_gpu.py): w, theta, counts, row list, lists
    out = _child(tmp_path, "fused", dict(CYTO_CACHE_FUSED="2"))
    assert out["fused"] == 8


# ---- the chain solver (mode = 1) ---------------------------------------------------------------------------------------------------

def _chain_instances():
    base = -(np.random.default_rng(9).random((200, 1000)) ** 3).astype(np.float32)          # (test_exception_columns_...)
    return {"uniform700": _uniform(700), "dup1000": np.repeat(base, 5, axis=0)}


CHAIN_OPTS = {
    "chain_variant1": dict(chain_variant=1), "chain_variant2": dict(chain_variant=2), "chain_variant3": dict(chain_variant=3),
    "augmentation1": dict(augmentation=1), "augmentation2": dict(augmentation=2, no_handover=1),
    "inject_exceptions5": dict(augmentation=2, no_handover=1, inject_exceptions=5),
    "inject_exceptions100": dict(augmentation=2, no_handover=1, inject_exceptions=100),
    "group_state_global_dense": dict(augmentation=1, group_state_global=1),
    "group_state_global_cached": dict(augmentation=2, no_handover=1, group_state_global=1),
    "aux_state_global": dict(augmentation=1, aux_state_global=1),
    "plain": dict(),
}


@pytest.mark.parametrize("variant", list(CHAIN_OPTS))
def test_chain_solver_variants(variant):
    opts = dict(mode=1, **CHAIN_OPTS[variant])
    for name, c in _chain_instances().items():
        o = _oracle(("chain", name), lambda: jv_oracle(c, np.float32))
        out = _eight(lambda: _lap_out(lap_solve(c, np.float32, return_info=True, opts=opts)), _lap_check(o))
        assert np.array_equal(np.sort(out["colsol"]), np.arange(len(c)))


# ---- float64 ----------------------------------------------------------------------------------------------------------------------

def _f64_case(n, opts, warm):
    c = _uniform(n).astype(np.float64)
    o = _oracle(("f64", n, warm), lambda: jv_oracle(c, np.float64, warm=warm))

    def call():
        g = lap_solve(c, np.float64, return_info=True, opts=opts)
        assert g["info"].f64_warm == (1 if warm else 0)
        return _lap_out(g)
    _eight(call, _lap_check(o))


@pytest.mark.parametrize("start", ["cold", "warm"])
@pytest.mark.parametrize("n", [3, 64, 300])
def test_float64_cold_and_warm(n, start):
    _f64_case(n, dict(mode=1) if start == "cold" else None, start == "warm")


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_float64_streaming_chain_variants_at_300(variant):
    _f64_case(300, dict(chain_variant=variant), False)


def test_float64_default_streaming_path_at_4100():
    _f64_case(4100, None, True)


# ---- certify, polish, exact ---------------------------------------------------------------------------------------------------------

def _near_tie():
    from tools import cross_unique
    return cross_unique.instance("typed", 2973, 5283, 4)           # (test_polish_recovers_the_unique_optimum_on_a_near_tie)


def test_certify_on_the_near_tie():
    c = _near_tie()
    n = len(c)
    o = _oracle(("wide", "near_tie", 0), lambda: jv_oracle_wide(c, np.float32))
    red = c.astype(np.float64) - o["v"].astype(np.float64)[None, :]
    viol = np.maximum(red[np.arange(n), o["rowsol"]] - red.min(1), 0.0)        # (test_float64_certificate_of_a_float32_solve)

    def call():
        g = lap_solve(c, np.float32, return_info=True, opts=dict(certify=1))
        i = g["info"]
        return dict(_lap_out(g), certified=int(i.certified), gap=float(i.gap_f64), gap_max=float(i.gap_max_f64), gap_rows=int(i.gap_rows))

    def check(out, tag):
        _lap_check(o)(out, tag)
        assert out["certified"] == 1 and out["gap_rows"] == int((viol > 0).sum()) and out["gap_max"] == viol.max(), tag
        assert abs(out["gap"] - viol.sum()) <= 1e-12 * max(1.0, viol.sum()), tag
    _eight(call, check)


def test_polish_on_the_near_tie():
    c = _near_tie()
    classic = _oracle(("chain", "near_tie"), lambda: jv_oracle(c, np.float32))
    o = _oracle(("f64warm", "near_tie"), lambda: jv_oracle(c.astype(np.float64), np.float64, warm=True))     # (test_float64_polish_...)
    assert np.array_equal(o["rowsol"], classic["rowsol"])                                                  # the unique optimum

    def call():
        g = lap_solve(c, np.float32, return_info=True, opts=dict(polish=1))
        assert g["info"].polished == 1 and g["info"].certified == 1
        return _lap_out(g)
    _eight(call, _lap_check(o, cast=np.float32))


def _exact_instance():
    from tools import instances
    rows = instances.typed_unique_cost(300, 1200, 11)[0]                         # (tests/test_lap_exact_gpu.py: the overflow pass)
    rowmap = np.repeat(np.arange(300), 4).astype(np.int32)
    return rows, rowmap


def _exact_reference(full):
    from scipy.optimize import linear_sum_assignment
    c64 = full.astype(np.float64)
    r, cc = linear_sum_assignment(c64)
    return dict(opt=float(c64[r, cc].sum()), wide=jv_oracle_wide(full, np.float32))


def _exact_check(full, ref, overflow):
    n = len(full)
    c64 = full.astype(np.float64)

    def check(out, tag):
        # the optimum of the float32 matrix (an independent exact solver's total), on the float32 solve's prices; a row the repair
        # left alone keeps its dual, a moved one has fl32(c - v) on its new column (tests/test_lap_exact_gpu.py)
        assert np.array_equal(np.sort(out["colsol"]), np.arange(n)) and np.array_equal(out["rowsol"][out["colsol"]], np.arange(n)), tag
        assert abs(float(c64[np.arange(n), out["rowsol"]].sum()) - ref["opt"]) <= 1e-12 * abs(ref["opt"]), tag
        assert abs(out["total"] - ref["opt"]) <= 1e-12 * abs(ref["opt"]), tag
        assert np.array_equal(out["v"], ref["wide"]["v"]), tag
        moved = out["rowsol"] != ref["wide"]["rowsol"]
        assert np.array_equal(out["u"][~moved], ref["wide"]["u"][~moved]), tag
        assert np.array_equal(out["u"][moved], full[np.flatnonzero(moved), out["rowsol"][moved]] - out["v"][out["rowsol"][moved]]), tag
        assert out["exact_status"] == 2 and out["edges"] > 0 and (out["overflow"] > 0 or not overflow), (tag, out["overflow"])
    return check


def _exact_out(g):
    i = g["info"]
    return dict(_lap_out(g), exact_status=int(i.exact_status), edges=int(i.exact_edges), overflow=int(i.exact_overflow_rows),
                changed=int(i.exact_changed_rows))


@pytest.mark.parametrize("slots", [16, 2])
@pytest.mark.parametrize("how", ["single", "rowmap", "batch"])
def test_exact_option(how, slots):
    # 2 slots per row: most rows overflow and are emitted again into a list of their own (b_list, b_csr)
    rows, rowmap = _exact_instance()
    full = rows[rowmap]
    ref = _oracle(("exact", "typed1200"), lambda: _exact_reference(full))
    opts = dict(exact=1 if slots == 16 else slots)
    check = _exact_check(full, ref, overflow=slots == 2)
    if how == "single":
        _eight(lambda: _exact_out(lap_solve(full, np.float32, return_info=True, opts=opts)), check)
    elif how == "rowmap":
        _eight(lambda: _exact_out(lap_solve_rows(rows, rowmap, return_info=True, opts=opts)), check)
    else:
        other = _uniform(300)
        ref2 = _oracle(("exact", "uniform300"), lambda: _exact_reference(other))

        def check_both(out, tag):
            check(out[0], tag + " problem 0")
            n = 300
            assert abs(float(other.astype(np.float64)[np.arange(n), out[1]["rowsol"]].sum()) - ref2["opt"]) <= 1e-12 * abs(ref2["opt"]), tag
            assert np.array_equal(out[1]["v"], ref2["wide"]["v"]) and out[1]["exact_status"] in (1, 2), tag
        _eight(lambda: [_exact_out(g) for g in lap_solve_batch([full, other], return_info=True, opts=opts)], check_both)


# ---- a batch ------------------------------------------------------------------------------------------------------------------------

def test_batch_of_mixed_sizes_two_at_a_time():
    sizes = [64, 64, 300, 65, 300, 1]
    costs = [np.random.default_rng(500 + b).random((n, n)).astype(np.float32) for b, n in enumerate(sizes)]
    oracles = [jv_oracle_wide(c, np.float32) for c in costs]

    def check(out, tag):
        for b, (g, o) in enumerate(zip(out, oracles)):
            _lap_check(o)(g, f"{tag} problem {b}")
    _eight(lambda: [_lap_out(g) for g in lap_solve_batch(costs, max_concurrent=2, return_info=True)], check)


# ---- other LAP inputs ---------------------------------------------------------------------------------------------------------------

def test_float32_solve_of_a_float64_host_matrix():
    c64 = np.random.default_rng(65).random((65, 65)) * 3.0 - 1.0              # (test_float64_host_matrix_is_narrowed_on_the_device)
    o = jv_oracle_wide(c64.astype(np.float32), np.float32)
    assert c64.flags.c_contiguous
    _eight(lambda: _lap_out(lap_solve(c64, np.float32, return_info=True)), _lap_check(o))         # cyto_lap_f32_from_f64


def _odd_pitch_unaligned(c, W):
    """The matrix on the device with a pitch that is no multiple of W and a base one element in; every element that is not data is
    NaN.  The library re-pitches it into a work buffer, whose own padding is the poison."""
    n = len(c)
    ld, _ = LY.pitch_and_lead(n, "odd_pitch", W)
    lead = 1
    host = np.full(lead + n * ld + LY.TAIL, np.nan, c.dtype)
    host[lead:lead + n * ld].reshape(n, ld)[:, :n] = c
    buf = _lib.DeviceBuffer.from_numpy(host)
    return buf, buf.ptr + lead * c.itemsize, ld


@pytest.mark.parametrize("n", [65, 301])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_device_resident_cost_is_repitched_into_poisoned_padding(dtype, n):
    c = _uniform(n).astype(dtype)
    assert n % 4 == 1
    o = jv_oracle_wide(c, np.float32) if dtype == np.float32 else jv_oracle(c, np.float64, warm=True)
    buf, ptr, ld = _odd_pitch_unaligned(c, 4 if dtype == np.float32 else 2)
    try:
        # (CYTO_ERR_NONFINITE would raise a ValueError: the padding is not a cost)
        _eight(lambda: _lap_out(lap_solve(None, dtype, return_info=True, device_ptr=ptr, n=n, ld=ld)), _lap_check(o))
    finally:
        buf.free()


# ---- the cost build -----------------------------------------------------------------------------------------------------------------

def _tied_counts(G, C, rng, dtype):
    x = rng.poisson(0.7, (G, C)).astype(np.float64)               # heavy ties for the ranks: most entries 0
    x[np.arange(C) % G, np.arange(C)] = 0                           # (no constant column: test_cost_precision_gpu._value_classes)
    x[(np.arange(C) + 1) % G, np.arange(C)] = 1 + np.arange(C) % 7
    return x.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.uint16], ids=["f64", "u16"])
@pytest.mark.parametrize("shape", [(33, 7), (1025, 131)], ids=["33x7", "1025x131"])
@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_transform_operand(transform, shape, dtype):
    G, C = shape
    tr = TRANSFORMS[transform]
    x = _tied_counts(G, C, np.random.default_rng(G + C), dtype)
    r64, delta = P.operand(x, tr, 0)

    def check(z, tag):
        pad = np.concatenate([z[G:].ravel(), z[:G, C:].ravel()]).view(np.uint32)
        assert not (pad != 0).any(), f"{tag}: {(pad != 0).sum()} padding words are not +0.0"
        assert np.isfinite(z[:G, :C]).all(), tag
        rep = P.ulp_report(z[:G, :C], r64, delta)
        assert rep["excess"] <= 0 and not rep["unexplained"], (tag, rep["excess"], rep["unexplained"], rep["where"])
    _eight(lambda: _transform(x, tr, 0, on_device=False), check)


@pytest.mark.parametrize("dtype", [np.float64, np.uint16], ids=["f64", "u16"])
@pytest.mark.parametrize("shape", [(33, 5, 7), (200, 130, 260)], ids=["33x5x7", "200x130x260"])
@pytest.mark.parametrize("metric", METRICS)
def test_cost_metric_contraction(metric, shape, dtype):
    G, S, C = shape
    rng = np.random.default_rng(G + S + C)
    sc, st = _tied_counts(G, C, rng, dtype), (_tied_counts(G, S, rng, np.float64) * 3 + rng.poisson(2.0, (G, S))).astype(dtype)
    slots = rng.integers(0, 4, S)
    slots[[0, S // 2, S - 1]] = [0, 3, 0]                          # uneven, zeros at both ends
    N, loc, ldc = int(slots.sum()), np.repeat(np.arange(S), slots), _up(C, 4) + 4
    ref = P.cost(metric, sc, st)[loc]

    def call():
        zsc = gcommon.StandardizedMatrix(sc, False, 0, metric)
        zst = gcommon.StandardizedMatrix(st, False, 0, metric)
        try:
            return _cost_metric(metric, zst, zsc, slots, N + 1, ldc)
        finally:
            zsc.buf.free()
            zst.buf.free()

    def check(buf, tag):
        assert (buf[:N, C:] == SENTINEL).all() and (buf[N] == SENTINEL).all(), f"{tag}: a store outside the N x C block"
        err = P.cost_error(metric, buf[:N, :C], ref)
        assert err.max() <= TOL, f"{tag}: max error {err.max():.3g}"
    _eight(call, check)


@pytest.mark.parametrize("dtype", [np.float64, np.uint16], ids=["f64", "u16"])
def test_normalize_data(dtype):
    x = _tied_counts(1025, 131, np.random.default_rng(4), dtype)
    x[:, 4] = 0                                                    # a column without counts: NaN -> 0
    want = ocost.normalize_data(x.astype(np.float64))

    def check(out, tag):
        assert out.dtype == np.float64 and (out[:, 4] == 0).all(), tag
        np.testing.assert_allclose(out, want, rtol=1e-12, atol=1e-12, err_msg=tag)       # (tests/test_cost_gpu.py::test_gv1_normalize_data)
    _eight(lambda: gcommon.normalize_data(x), check)


def test_csc_to_dense():
    import scipy.sparse as sp
    sc = _tied_counts(200, 131, np.random.default_rng(5), np.float32)

    def call():
        buf, G, C, ld = gcommon.sparse_to_device(sp.csc_matrix(sc))           # cyto_csc_to_dense_f32
        try:
            assert (G, C) == sc.shape
            return buf.to_numpy((G, ld), np.float32)
        finally:
            buf.free()

    def check(out, tag):
        assert np.array_equal(out[:, :131].view(np.uint32), sc.view(np.uint32)) and not out[:, 131:].view(np.uint32).any(), tag
    _eight(call, check)


def _eps(metric, ref):
    return TOL * (float(np.abs(ref).max()) if metric == "Euclidean" else 1.0)          # (tests/test_cost_precision_gpu.py)


def _lsap_optimum(ref, slots):
    from scipy.optimize import linear_sum_assignment
    full = ref[np.repeat(np.arange(len(slots)), slots)]
    r, c = linear_sum_assignment(full)
    return float(full[r, c].sum())


def _assignment_check(ref, slots, idx=None):
    """A spot per cell against the float64 cost: the slot counts, and a total within the cost build's tolerance of an independent
    exact solver's optimum (tests/test_cost_precision_gpu.py::test_fused_and_context_totals_on_the_float64_cost)."""
    idx = np.arange(ref.shape[1]) if idx is None else idx
    sub = ref[:, idx]
    best = _lsap_optimum(sub, slots)

    def check(mapped, tag, eps):
        assert np.array_equal(np.bincount(mapped, minlength=len(slots)), slots), tag
        mine = float(sub[mapped, np.arange(len(idx))].sum())
        assert best - 1e-9 * abs(best) <= mine <= best + 2 * len(idx) * eps, (tag, mine, best)
    return check


@pytest.mark.parametrize("dtype", [np.float64, np.uint16], ids=["f64", "u16"])
@pytest.mark.parametrize("metric", METRICS)
def test_assign_metric(metric, dtype):
    rng = np.random.default_rng(7)
    G, S, k = 300, 40, 3                                           # (__graft_entry__.smoke)
    C = S * k
    sc = rng.poisson(3.0, (G, C)).astype(dtype)
    st = rng.poisson(9.0, (G, S)).astype(dtype)
    slots = np.full(S, k, np.int64)
    ref = P.cost(metric, sc, st)
    check_spots = _assignment_check(ref, slots)
    L = _lib.lib()

    def call():
        mapped = np.empty(C, np.int64)
        total = ctypes.c_double()
        info = _lib.AssignInfo()
        if dtype == np.float64:                                    # cyto_assign_metric itself: float64 host matrices
            _lib.check(L.cyto_assign_metric(gcommon.METRICS[metric], G, C, S, sc.ctypes.data, st.ctypes.data, slots.ctypes.data, 0,
                                            mapped.ctypes.data, ctypes.byref(total), ctypes.byref(info), 0))
            return dict(mapped=mapped, total=total.value)
        m, t, _ = gcyto.assign_pearson(sc, st, slots, already_normalized=False, return_info=True, distance_metric=metric)
        return dict(mapped=m, total=t)
    _eight(call, lambda out, tag: check_spots(out["mapped"], tag, _eps(metric, ref)))


@pytest.mark.parametrize("dtype", [np.float64, np.uint16], ids=["f64", "u16"])
@pytest.mark.parametrize("max_concurrent", [1, 2])
def test_expression_context_chunks(max_concurrent, dtype):
    # three chunks of one call -- a batch with row maps on some problems: the first chunk has a cell per spot (no map), the second
    # two per spot, the third four per spot on 9 spots and none on the other 15; against the per-chunk path and the float64 cost, at
    # spot level (test_expression_context_chunks_equal_per_chunk_uploads)
    rng = np.random.default_rng(17)
    G, S, C = 90, 24, 132
    sc = rng.poisson(2.0, (G, C)).astype(dtype)
    st = rng.poisson(8.0, (G, S)).astype(dtype)
    ref = P.cost("Pearson_correlation", sc, st)
    eps = _eps("Pearson_correlation", ref)
    chunks = []
    for k, size in enumerate((24, 48, 36)):
        idx = np.sort(rng.permutation(C)[:size])
        slots = np.full(S, size // S, np.int64)
        if k == 2:
            slots = np.zeros(S, np.int64)
            slots[rng.permutation(S)[:9]] = 4                       # 15 spots without a cell
        assert slots.sum() == size
        chunks.append((idx, slots))
    checks = [_assignment_check(ref, slots, idx) for idx, slots in chunks]

    def call():
        with gcyto.ExpressionContext(sc, st, False) as ctx:
            both = ctx.assign_chunks(chunks, max_concurrent=max_concurrent)
            one = [ctx.assign_chunk(idx, slots) for idx, slots in chunks]
        per_chunk = [gcyto.assign_pearson(sc[:, idx], st, slots, already_normalized=False) for idx, slots in chunks]
        return dict(both=both, one=one, per_chunk=per_chunk)

    def check(out, tag):
        for k in range(3):
            assert np.array_equal(out["both"][k], out["one"][k]) and np.array_equal(out["both"][k], out["per_chunk"][k]), (tag, k)
            checks[k](out["both"][k], f"{tag} chunk {k}", eps)
    _eight(call, check)


# ---- the other device paths ---------------------------------------------------------------------------------------------------------

def test_mt19937_fill():
    def call():
        np.random.seed(77)                                         # (tests/test_downsample_gpu.py::test_raw_fill_equals_numpy_words)
        np.random.randint(0, 2**32, 624 + 227, dtype=np.uint32)
        st = np.random.get_state()
        got = gcommon.mt19937_fill(5000)
        after = np.random.get_state()
        np.random.set_state(st)
        want = np.random.randint(0, 2**32, 5000, dtype=np.uint32)
        assert np.array_equal(got, want) and after[2] == np.random.get_state()[2] and np.array_equal(after[1], np.random.get_state()[1])
        return got
    _eight(call)


def test_downsample():
    from test_downsample_gpu import _check
    rng = np.random.default_rng(3)
    x = rng.poisson(rng.lognormal(0, 1.5, (257, 1)) * 0.5, (257, 65)).astype(np.int64)           # (test_random_shapes)
    x[:, ::3] //= 4
    _eight(lambda: _check(x, 100, 13))                              # against the host downsample: values and numpy's state afterwards


def test_placeholders_in_several_blocks():
    from test_placeholders_gpu import _check
    G, short, n = 65, 130, 7                                        # (test_blocks: 44 blocks of 3 cells)
    own = np.random.default_rng(7).integers(0, 1000, (G, n))
    _eight(lambda: _check(own, short, seed=21, rbuf_bytes=4 * G * 3)[0])


def test_table_read_and_fetch(tmp_path):
    from test_read_table_gpu import _device, _frame
    p = tmp_path / "t.tsv"
    _frame(np.random.default_rng(26), 37, 53, "mixed").to_csv(p, sep="\t")
    _eight(lambda: _device(p))                                      # against read_file (pandas), values bit for bit


def test_mtx_write_in_small_blocks(tmp_path):
    from cytospace_amd.post_processing import write_mtx_device
    from test_mtx_writer_gpu import scipy_bytes, spread_values
    rng = np.random.default_rng(20)
    frame = pd.DataFrame(spread_values(rng, (37, 300), np.int32, 0.3))
    columns = rng.integers(0, 300, 1111)
    want = scipy_bytes(frame, columns)
    p = str(tmp_path / "m.mtx")

    def call():
        info = write_mtx_device(p, frame, columns, block_bytes=300, return_info=True)
        assert info["path"] == "device" and info["blocks"] > 1, info
        return open(p, "rb").read()

    def check(got, tag):
        assert got == want, tag
    _eight(call, check)
