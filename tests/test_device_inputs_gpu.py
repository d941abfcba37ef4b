"""Device-resident inputs: WHERE the bytes lie.  Every other GPU module pins values; this one pins pitch, padding and base alignment
(include/cytohip.h, "Device inputs and caller streams"): any ld >= the width and any base are accepted, the bytes outside the
n x n (G x C) block are never interpreted and never written.

Every matrix goes up in a named layout of tests/_layouts.py (tight, padded, wide, double, odd_pitch, offset_base, quad_offset_base)
with every element that is not data set to a poison: -1e30, NaN, -inf (integer types: the type's maximum).  A kernel that steps rows
by the padded width instead of ld, that lets a padding element into a minimum, a column sum or a rank, or that flags it as a
non-finite cost changes the answer.  Every case asserts
  1. LAPs: indices and duals bit for bit those of the CPU oracle (jv_oracle / jv_oracle_wide), the total within the suite's tolerance
     of the oracle's and equal to the host-layout solve's; transforms, contractions, context solves: the bits of the same call on a
     contiguous host copy (the tight layout for the contraction, whose operands only ever live on the device);
  2. the semantic counters (STAT_KEYS / WIDE_KEYS of test_lap_gpu.py) equal the host-layout solve's: the same path ran;
  3. no CYTO_ERR_NONFINITE (a ValueError) because of the padding -- while a real NaN / +inf in the last column still raises;
  4. the caller's whole buffer is byte-identical afterwards (compared as uint8: it holds NaN).
The oracle of an instance is computed once and shared; failures of one case are collected and reported together.
"""
import ctypes
import types

import numpy as np
import pytest

import _layouts as LY
from cytospace_amd import _lib
from cytospace_amd import common as gcommon
from cytospace_amd import cytospace as gcyto
from cytospace_amd.lap import lap_solve, lap_solve_rows
from oracle.jv import jv_oracle, jv_oracle_wide
from test_cost_precision_gpu import DTYPES, METRICS, SENTINEL, TRANSFORMS, _cost_metric, _counts, _up, _value_classes
from test_lap_gpu import STAT_KEYS, WIDE_KEYS

pytestmark = pytest.mark.gpu

WIDE_STAT_KEYS = [kg for kg, _ in WIDE_KEYS]


class Resident:
    """A matrix uploaded in a named layout.  ptr: the device address of its base; ld: its pitch."""

    def __init__(self, matrix, layout, W, poison, skip_rows=()):
        self.host, self.lead, self.ld = LY.build(matrix, layout, W, poison, skip_rows)
        self.buf = _lib.DeviceBuffer.from_numpy(self.host)
        assert self.buf.ptr % LY.ALLOC_ALIGN == 0
        self.ptr = self.buf.ptr + self.lead * self.host.itemsize

    def untouched(self):
        back = self.buf.to_numpy(self.host.shape, self.host.dtype)
        return np.array_equal(back.view(np.uint8), self.host.view(np.uint8))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.buf.free()


def _poison_name(p):
    return "nan" if np.isnan(p) else "-inf" if np.isinf(p) else "-1e30"


# ---- LAP --------------------------------------------------------------------------------------------------------------------

LAP_N = (1, 2, 5, 63, 301, 1000, 1001)
F32_VARIANTS = {                       # name -> (cyto_lap_opts or None: cyto_lap_f32, the oracle's restatement)
    "default": (None, "wide"),
    "chain": (dict(mode=1), "chain"),
    "chain_variant1": (dict(mode=1, chain_variant=1), "chain"),
    "chain_variant2": (dict(mode=1, chain_variant=2), "chain"),
    "chain_variant3": (dict(mode=1, chain_variant=3), "chain"),
    "augmentation1": (dict(mode=1, augmentation=1), "chain"),
    "augmentation2": (dict(mode=1, augmentation=2, no_handover=1), "chain"),
}
F64_VARIANTS = {"cold_chain": (dict(mode=1), "chain"), "warm": (None, "warm")}

_ORACLE = {}


def _cost(n, dtype):
    c = np.random.default_rng(900 + n).random((n, n))
    return c.astype(np.float32) if dtype == np.float32 else c


def _oracle(name, c, dtype, kind):
    key = (name, np.dtype(dtype).name, kind)
    if key not in _ORACLE:
        _ORACLE[key] = (jv_oracle_wide(c, np.float32, max_rounds=-1) if kind == "wide" else
                        jv_oracle(c, dtype, warm=True) if kind == "warm" else jv_oracle(c, dtype))
    return _ORACLE[key]


def _counter_keys(kind):
    return WIDE_STAT_KEYS if kind == "wide" else STAT_KEYS


def _host_equals_oracle(h, o, kind, dtype):
    """The host-layout solve against the oracle, as test_lap_gpu.py's _check / _check_wide / _check_warm have it."""
    for k in ("rowsol", "colsol", "v", "u"):
        assert np.array_equal(h[k], o[k]), ("host layout", k)
    tol = 1e-9 if kind == "warm" else 1e-5
    assert abs(h["total"] - o["total"]) <= tol * max(1.0, abs(o["total"]))
    hd, od = h["info"].as_dict(), o["stats"].as_dict()
    assert hd["wide"] == (1 if kind == "wide" else 0) and hd["f64_warm"] == (1 if kind == "warm" else 0)
    for kg, ko in (WIDE_KEYS if kind == "wide" else [(k, k) for k in STAT_KEYS]):
        assert hd[kg] == od[ko], ("host layout", kg, hd[kg], od[ko])


def _device_equals(g, h, o, kind, tag, failures):
    """A device-layout solve against the oracle (bits) and the host-layout solve (counters, total)."""
    for k in ("rowsol", "colsol", "v", "u"):
        if not np.array_equal(g[k], o[k]):
            failures.append(f"{tag}: {k} differs from the oracle in {(g[k] != o[k]).sum()} of {len(o[k])} entries")
    if g["total"] != h["total"]:
        failures.append(f"{tag}: total {g['total']!r} != the host layout's {h['total']!r}")
    gd, hd = g["info"].as_dict(), h["info"].as_dict()
    for k in _counter_keys(kind) + ["wide", "f64_warm"]:
        if gd[k] != hd[k]:
            failures.append(f"{tag}: counter {k} = {gd[k]}, host layout {hd[k]}")


def _solve_layouts(c, dtype, W, opts, kind, name, layouts=LY.LAYOUTS, poisons=LY.POISONS):
    n = len(c)
    if kind == "warm" and n < 2:
        kind = "chain"          # one row: nothing to warm-start, the library's default float64 solve is the cold one (lap_solve_f64: n >= 2)
    o = _oracle(name, c, dtype, kind)
    h = lap_solve(c, dtype, return_info=True, opts=opts)
    _host_equals_oracle(h, o, kind, dtype)
    failures = []
    for layout in layouts:
        for poison in poisons:
            tag = f"n={n} {layout} (ld {LY.pitch_and_lead(n, layout, W)[0]}) poison {_poison_name(poison)}"
            with Resident(c, layout, W, poison) as r:
                try:
                    g = lap_solve(None, dtype, return_info=True, device_ptr=r.ptr, n=n, ld=r.ld, opts=opts)
                except ValueError as e:                   # CYTO_ERR_NONFINITE / BAD_ARG: the padding was taken for a cost
                    failures.append(f"{tag}: {e}")
                    continue
                _device_equals(g, h, o, kind, tag, failures)
                if not r.untouched():
                    failures.append(f"{tag}: the caller's buffer changed")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:20])


@pytest.mark.parametrize("n", LAP_N)
@pytest.mark.parametrize("variant", list(F32_VARIANTS))
def test_lap_f32_on_device_layouts(variant, n):
    # cyto_lap_f32 (default: the wide solver) and cyto_lap_f32_opts: the chain solver, its large-n variants and both augmentations
    # forced as test_large_n_code_path_forced_at_small_n forces them.  padded / wide / double with an aligned base are used in place;
    # tight (n % 4 != 0), odd_pitch and the offset bases go through the re-pitch, whose own padding is stale block-cache content
    opts, kind = F32_VARIANTS[variant]
    _solve_layouts(_cost(n, np.float32), np.float32, 4, opts, kind, f"uniform{n}")


@pytest.mark.parametrize("poison", LY.POISONS, ids=_poison_name)
@pytest.mark.parametrize("n", LAP_N + (302,))
@pytest.mark.parametrize("variant", list(F64_VARIANTS))
def test_lap_f64_on_device_layouts(variant, n, poison):
    # cyto_lap_f64: rows in pairs (VW = 2: in place when ld % 2 == 0 and the base is 16-byte aligned); the cold chain, and the default
    # warm start, which narrows the matrix to float32 on the device for the wide solve.  (A case per poison: the cold chain takes
    # a quarter of a second at n = 1000.)
    opts, kind = F64_VARIANTS[variant]
    _solve_layouts(_cost(n, np.float64), np.float64, 2, opts, kind, f"uniform{n}", poisons=(poison,))


def _rowmap_case(n):
    """Slots of 1-5 (the first at least 2 when n allows it) and stored rows the map skips, so that nu < n for n >= 2."""
    rng = np.random.default_rng(3000 + n)
    slots = []
    while sum(slots) < n:
        lo = 2 if not slots else 1
        slots.append(min(int(rng.integers(lo, 6)), n - sum(slots)))
    used = len(slots)
    nskip = min(max(0, n - 1 - used), 1 + used // 3)
    nu = used + nskip
    skip = np.sort(rng.choice(nu, nskip, replace=False))
    used_rows = np.setdiff1d(np.arange(nu), skip)
    rowmap = np.repeat(used_rows, slots).astype(np.int32)
    rows = -(rng.random((nu, n)) ** 3).astype(np.float32)
    rows[skip] = 0.0
    return rows, rowmap, skip


@pytest.mark.parametrize("n", LAP_N)
@pytest.mark.parametrize("variant", ["default", "chain"])
def test_lap_f32_rowmap_on_device_layouts(variant, n):
    # cyto_lap_f32_rowmap with pitch > n: every distinct row stored once, rows no LAP row names filled with poison; the oracle solves
    # the materialised rows[rowmap]
    opts, kind = F32_VARIANTS[variant]
    rows, rowmap, skip = _rowmap_case(n)
    nu = len(rows)
    assert len(rowmap) == n and (nu < n or n == 1) and not np.isin(skip, rowmap).any()
    full = rows[rowmap]
    o = _oracle(f"rowmap{n}", full, np.float32, kind)
    h = lap_solve_rows(rows, rowmap, return_info=True, opts=opts)
    _host_equals_oracle(h, o, kind, np.float32)
    failures = []
    for layout in LY.LAYOUTS:
        for poison in LY.POISONS:
            tag = f"n={n} nu={nu} {layout} poison {_poison_name(poison)}"
            with Resident(rows, layout, 4, poison, skip_rows=skip) as r:
                try:
                    g = lap_solve_rows(None, rowmap, return_info=True, device_ptr=r.ptr, nu=nu, ld=r.ld, opts=opts)
                except ValueError as e:
                    failures.append(f"{tag}: {e}")
                    continue
                _device_equals(g, h, o, kind, tag, failures)
                if not r.untouched():
                    failures.append(f"{tag}: the caller's buffer changed")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:20])


def _certificate_instances():
    from tools import cross_unique
    return {"instance283": lambda: cross_unique.instance("typed", 2973, 5283, 4),       # n % 4 == 1, gap > 0
            "uniform1500": lambda: np.random.default_rng(41).random((1500, 1500)).astype(np.float32)}


CERT_KEYS = ("certified", "gap_f64", "gap_max_f64", "gap_rows", "polished", "exact_status", "exact_edges", "exact_free_rows",
             "exact_changed_rows", "exact_overflow_rows")


@pytest.mark.parametrize("option", ["certify", "polish", "exact"])
@pytest.mark.parametrize("instance", ["instance283", "uniform1500"])
def test_certificate_polish_and_exact_on_device_layouts(instance, option):
    # the passes behind the solve read the caller's matrix again: dual_gap_rows (its float4 sweep only where row and v are 16-byte
    # aligned), near_tight_rows, the widening of the polish.  Everything they report must equal the host-layout run's
    c = np.ascontiguousarray(_certificate_instances()[instance](), dtype=np.float32)
    n = len(c)
    opts = {option: 1}
    h = lap_solve(c, np.float32, return_info=True, opts=opts)
    hd = h["info"].as_dict()
    assert hd["certified"] == 1
    if instance == "instance283":
        assert n % 4 == 1 and hd["gap_f64"] > 0.0 and hd["gap_rows"] > 0
        assert option != "polish" or hd["polished"] == 1
        assert option != "exact" or (hd["exact_status"] == 2 and hd["exact_changed_rows"] > 0)
    failures = []
    for layout in ("padded", "wide", "offset_base"):
        for poison in LY.POISONS:
            tag = f"{instance} {option} {layout} poison {_poison_name(poison)}"
            with Resident(c, layout, 4, poison) as r:
                try:
                    g = lap_solve(None, np.float32, return_info=True, device_ptr=r.ptr, n=n, ld=r.ld, opts=opts)
                except ValueError as e:
                    failures.append(f"{tag}: {e}")
                    continue
                gd = g["info"].as_dict()
                for k in ("rowsol", "colsol", "u", "v"):
                    if not np.array_equal(g[k], h[k]):
                        failures.append(f"{tag}: {k} differs from the host layout's in {(g[k] != h[k]).sum()} entries")
                if g["total"] != h["total"]:
                    failures.append(f"{tag}: total {g['total']!r} != {h['total']!r}")
                for k in CERT_KEYS + tuple(WIDE_STAT_KEYS):
                    if gd[k] != hd[k]:
                        failures.append(f"{tag}: {k} = {gd[k]!r}, host layout {hd[k]!r}")
                if not r.untouched():
                    failures.append(f"{tag}: the caller's buffer changed")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:20])


@pytest.mark.parametrize("variant", ["default", "chain"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_real_nonfinite_cost_in_the_last_column_is_still_rejected(bad, variant):
    # the negative control of (3): n % 4 == 1, so column n - 1 opens the last quad, whose other three elements are padding
    n = 301
    opts, _ = F32_VARIANTS[variant]
    for row in (0, 150, n - 1):
        c = _cost(n, np.float32).copy()
        c[row, n - 1] = bad
        for poison in LY.POISONS:
            with Resident(c, "padded", 4, poison) as r:
                assert r.ld == 304 and r.ptr % 16 == 0
                with pytest.raises(ValueError):
                    lap_solve(None, np.float32, device_ptr=r.ptr, n=n, ld=r.ld, opts=opts)


# ---- transforms (cyto_transform, x_on_device = 1) -----------------------------------------------------------------------------

TRANSFORM_SHAPES = ((33, 4), (257, 256), (257, 260), (300, 255), (1030, 1028))
TRANSFORM_LAYOUTS = ("tight", "wide", "double", "odd_pitch", "offset_base", "quad_offset_base")


def _run_transform(tr, G, C, x, ldx, code, on_device, already, extra):
    """cyto_transform into a z buffer of Gpad x ldz floats, ldz = round_up(C, 128) + extra, pre-filled with 0xFF bytes and followed by
    one more row of them.  Returns the (Gpad + 1) x ldz words."""
    Gpad, ldz = _up(G, 32), _up(C, 128) + extra
    z = _lib.DeviceBuffer.from_numpy(np.full((Gpad + 1) * ldz * 4, 0xFF, np.uint8))
    try:
        _lib.check(_lib.lib().cyto_transform(tr, G, C, x, ldx, code, on_device, already, z.ptr, ldz, Gpad, 0, None))
        return z.to_numpy((Gpad + 1, ldz), np.uint32)
    finally:
        z.free()


@pytest.mark.parametrize("already", [0, 1])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_transform_of_device_layouts_gives_the_host_bits(transform, dtype, already):
    """The four-column kernels run where C % 4 == 0, ldx % 4 == 0 and the base is aligned for a quad of the type (16 bytes for
    float32 / float64, 8 for uint16, 4 for uint8) -- tight, wide and double at C = 4, 256, 260, 1028, and quad_offset_base for the
    integer types; everything else takes the one-column kernels.  Both must give the bits of the host run (ldx = C), and the poison
    in the pitch padding must not move a column sum, a moment or a rank.

    The output contract of cyto_transform (cost.hip): of the caller's Gpad x ldz buffer the G x C block holds the operand, every other
    element is +0.0 -- columns C ... ldz of the first G rows and the rows G ... Gpad in full, whatever ldz >= C is -- and nothing
    beyond Gpad x ldz is written.  So with ldz = round_up(C, 128) + 128 the extra 128 columns come back zero, and the row of 0xFF bytes
    behind the buffer comes back untouched."""
    tr, (dt, code) = TRANSFORMS[transform], DTYPES[dtype]
    rng = np.random.default_rng(2000 + 100 * tr + 10 * code + already)
    poisons = LY.POISONS if np.dtype(dt).kind == "f" else LY.POISONS[:1]        # (integer types: one poison, the maximum)
    failures = []
    for G, C in TRANSFORM_SHAPES:
        x = np.ascontiguousarray(_value_classes(G, C, dt, tr, already, rng))
        Gpad = _up(G, 32)
        ref = _run_transform(tr, G, C, x.ctypes.data, C, code, 0, already, 0)
        assert (ref[Gpad] == 0xFFFFFFFF).all() and not ref[G:Gpad].any() and not ref[:G, C:].any()
        for layout in TRANSFORM_LAYOUTS:
            # every poison with the usual ldz = round_up(C, 128); the wider output once, with NaN (integer types: the maximum)
            for poison, extra in [(p, 0) for p in poisons] + [(poisons[len(poisons) // 2], 128)]:
                tag = f"G={G} C={C} {layout} poison {_poison_name(poison)} ldz=+{extra}"
                with Resident(x, layout, 4, poison) as r:
                    try:
                        out = _run_transform(tr, G, C, r.ptr, r.ld, code, 1, already, extra)
                    except ValueError as e:
                        failures.append(f"{tag}: {e}")
                        continue
                    if not np.array_equal(out[:G, :C], ref[:G, :C]):
                        failures.append(f"{tag}: {(out[:G, :C] != ref[:G, :C]).sum()} words of the operand differ from the host run's "
                                        f"(columns {np.flatnonzero((out[:G, :C] != ref[:G, :C]).any(0))[:8]})")
                    if out[:G, C:].any() or out[G:Gpad].any():
                        failures.append(f"{tag}: {np.count_nonzero(out[:G, C:]) + np.count_nonzero(out[G:Gpad])} padding words are not +0.0")
                    if not (out[Gpad] == 0xFFFFFFFF).all():
                        failures.append(f"{tag}: a store beyond Gpad x ldz")
                    if not r.untouched():
                        failures.append(f"{tag}: the caller's input changed")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:20])


# ---- the contraction (cyto_cost_metric) --------------------------------------------------------------------------------------

def _widened(z):
    """A StandardizedMatrix's operand in a buffer of pitch ld + 128 with NaN in the 128 extra columns."""
    host = z.buf.to_numpy((z.Gpad, z.ld), np.float32)
    wide = np.full((z.Gpad, z.ld + 128), np.nan, np.float32)
    wide[:, :z.ld] = host
    return types.SimpleNamespace(Gpad=z.Gpad, C=z.C, ld=z.ld + 128, buf=_lib.DeviceBuffer.from_numpy(wide), host=wide)


@pytest.mark.parametrize("G", [32, 97])
@pytest.mark.parametrize("metric", METRICS)
def test_contraction_with_wide_operands_and_a_wide_output(metric, G):
    # operands of pitch round_up(., 128) + 128 with NaN in the extra columns, the cost of pitch round_up(C, 4) + 8 with a sentinel in
    # the extra columns and in one more row: the bits of the tight layout, the sentinel intact, the operands unchanged
    S, C = 130, 260
    rng = np.random.default_rng(40 + G)
    sc, st = _counts(G, C, rng, 0.3), _counts(G, S, rng, 3.0)
    zsc = gcommon.StandardizedMatrix(sc, False, 0, metric)
    zst = gcommon.StandardizedMatrix(st, False, 0, metric)
    wsc = wst = None
    try:
        tight = _cost_metric(metric, zst, zsc, np.ones(S), S, _up(C, 4))
        assert np.isfinite(tight[:, :C]).all() and not (tight[:, :C] == SENTINEL).any()
        wsc, wst = _widened(zsc), _widened(zst)
        ldc = _up(C, 4) + 8
        got = _cost_metric(metric, wst, wsc, np.ones(S), S + 1, ldc)
        assert np.array_equal(got[:S, :C].view(np.uint32), tight[:, :C].view(np.uint32)), \
            f"{(got[:S, :C].view(np.uint32) != tight[:, :C].view(np.uint32)).sum()} entries differ from the tight layout's"
        assert (got[:S, C:] == SENTINEL).all() and (got[S] == SENTINEL).all()
        for w in (wsc, wst):
            assert np.array_equal(w.buf.to_numpy(w.host.shape, np.float32).view(np.uint32), w.host.view(np.uint32))
    finally:
        for z in (zsc, zst, wsc, wst):
            if z is not None:
                z.buf.free()


# ---- the context (cyto_ctx_create_ex, on_device = 1) -------------------------------------------------------------------------

def _device_context(rsc, rst, G, C, S, code, metric, already):
    ctx = gcyto.ExpressionContext.__new__(gcyto.ExpressionContext)
    ctx._h, ctx.bcast_ms, ctx.G, ctx.C, ctx.S = ctypes.c_void_p(), None, G, C, S
    msc, mst = _lib.Matrix(), _lib.Matrix()
    msc.data, msc.ld, msc.is_f64, msc.on_device = rsc.ptr, rsc.ld, code, 1
    mst.data, mst.ld, mst.is_f64, mst.on_device = rst.ptr, rst.ld, code, 1
    ms = ctypes.c_double()
    _lib.check(_lib.lib().cyto_ctx_create_ex(gcommon.METRICS[metric], G, ctypes.byref(msc), C, ctypes.byref(mst), S, already, None, 0, 0,
                                             0, ctypes.byref(ctx._h), ctypes.byref(ms)))
    return ctx


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("metric", METRICS)
def test_context_of_device_matrices_equals_the_host_context(metric, dtype):
    # G, S, C and the two chunks of test_expression_context_chunks_equal_per_chunk_uploads; raw counts (every dtype holds them)
    dt, code = DTYPES[dtype]
    rng = np.random.default_rng(17)
    G, S, C = 90, 24, 60
    sc = rng.poisson(2.0, (G, C)).astype(dt)
    st = rng.poisson(8.0, (G, S)).astype(dt)
    chunks = [(rng.permutation(C)[:20], np.array([3, 0, 5, 2, 0, 4, 1, 0, 5]), rng.permutation(S)[:9]),
              (np.arange(10, 58), np.full(S, 2), None)]
    with gcyto.ExpressionContext(sc, st, False, 0, metric) as ctx:
        want = [ctx.assign_chunk(i, s, j, return_info=True) for i, s, j in chunks]
    poisons = LY.POISONS if np.dtype(dt).kind == "f" else LY.POISONS[:1]
    for layout in ("wide", "odd_pitch"):
        for poison in poisons:
            with Resident(sc, layout, 4, poison) as rsc, Resident(st, layout, 4, poison) as rst:
                with _device_context(rsc, rst, G, C, S, code, metric, 0) as ctx:
                    for (i, s, j), (mapped, total, info) in zip(chunks, want):
                        got, total2, info2 = ctx.assign_chunk(i, s, j, return_info=True)
                        tag = (metric, dtype, layout, _poison_name(poison))
                        assert np.array_equal(got, mapped) and total2 == total, tag
                        assert info2.gemm_flops == info.gemm_flops, tag
                        for k in WIDE_STAT_KEYS:
                            assert getattr(info2.lap, k) == getattr(info.lap, k), (tag, k)
                assert rsc.untouched() and rst.untouched(), (metric, dtype, layout)
