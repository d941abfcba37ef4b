"""Caller streams: every entry point with a `void *stream` parameter must order its work behind what the caller already queued on
that stream, and return with its work complete (include/cytohip.h, "Device inputs and caller streams").

The in-flight input.  On one non-blocking stream s of the test's own:
  1. the device buffer the library will read holds a DECOY: a finite matrix of the payload's shape with a different answer (asserted on
     the host), so a wrong read gives the decoy's answer or a mixture and can never leave the buffer;
  2. a delay is queued on s: a chain of device-to-device copies between two scratch buffers, calibrated once per module to take at
     least 20 ms (scratch: 2 x 256 MiB);
  3. behind it, the device-to-device copy that overwrites the decoy with the payload (uploaded beforehand, synchronously, into another
     buffer);
  4. the entry point is called with stream = s at once, without synchronising.
The result must be the payload's: the CPU oracle's bits for the LAPs (cyto_lap_f32, cyto_lap_f32_opts, cyto_lap_f64,
cyto_lap_f32_rowmap), numpy's own for the views of a resident table (cyto_select: src[ix_(rows, cols)].astype; cyto_value_range: the
payload's minimum, maximum and counts), the bits of the same call on the NULL stream with settled inputs for the rest (cyto_transform,
cyto_cost_metric; cyto_csc_to_dense_f32 has host inputs).  Device outputs are read right after the call with plain cyto_memcpy_d2h (a
synchronous copy on the NULL stream, which a non-blocking stream does not wait for): they must be complete.

The premise is a condition, not a skip: right before the call hipStreamQuery(s) must say not-ready, and the event-measured delay must
be at least ten times the host-measured gap between the last enqueue's return and the library call -- else the test FAILS.

The HIP runtime is bound by tests/_hiprt.py (the copy libcytohip.so loaded).  One process, one extra stream.
"""
import ctypes
import time
import types

import numpy as np
import pytest

import _hiprt as hip
from cytospace_amd import _lib
from cytospace_amd import common as gcommon
from cytospace_amd.lap import lap_solve, lap_solve_rows
from oracle.jv import jv_oracle, jv_oracle_wide

pytestmark = pytest.mark.gpu

SCRATCH_BYTES = 256 << 20        # each of the two scratch buffers of the delay chain (1 GiB in total is the limit)
MIN_DELAY_MS = 20.0
SENTINEL = np.float32(-12345.25)


def _up(x, m):
    return -(-x // m) * m


class Flight:
    """The stream, the delay chain and the bookkeeping of the premise."""

    def __init__(self):
        self.s = hip.stream_create()
        self.a = _lib.DeviceBuffer(SCRATCH_BYTES)
        self.b = _lib.DeviceBuffer(SCRATCH_BYTES)
        self.e0, self.e1 = hip.event_create(), hip.event_create()
        self.copies, self.chain_ms = 0, 0.0

    def _chain(self, k):
        for i in range(k):
            dst, src = (self.b, self.a) if i % 2 == 0 else (self.a, self.b)
            hip.memcpy_d2d_async(dst.ptr, src.ptr, SCRATCH_BYTES, self.s)

    def calibrate(self):
        """Time a short chain with events and lengthen it until it takes MIN_DELAY_MS (with a quarter to spare)."""
        k = 8
        for _ in range(6):
            hip.event_record(self.e0, self.s)
            self._chain(k)
            hip.event_record(self.e1, self.s)
            hip.event_synchronize(self.e1)
            ms = hip.event_elapsed_ms(self.e0, self.e1)
            if ms >= 1.25 * MIN_DELAY_MS:
                break
            k = min(20000, int(k * 1.5 * MIN_DELAY_MS / max(ms, 1e-3)) + 1)
        self.copies, self.chain_ms = k, ms
        assert ms >= MIN_DELAY_MS, f"a chain of {k} copies of {SCRATCH_BYTES >> 20} MiB takes only {ms:.2f} ms"
        print(f"\n[in-flight] calibration: {k} device-to-device copies of {SCRATCH_BYTES >> 20} MiB take {ms:.1f} ms")

    def run(self, name, overwrites, call):
        """Queue the delay and the copies (dst, src, bytes) that put the payloads in place, call the library at once, and return
        (what `call` returned, a function that checks the premise).  The caller reads its device outputs BEFORE checking the
        premise: that check waits for the delay's event."""
        hip.event_record(self.e0, self.s)
        self._chain(self.copies)
        hip.event_record(self.e1, self.s)
        for dst, src, nbytes in overwrites:
            hip.memcpy_d2d_async(dst, src, nbytes, self.s)
        t_enqueued = time.perf_counter()
        ready = hip.stream_ready(self.s)
        t_call = time.perf_counter()
        out = call(self.s)
        t_returned = time.perf_counter()

        def premise():
            hip.event_synchronize(self.e1)
            delay = hip.event_elapsed_ms(self.e0, self.e1)
            gap = (t_call - t_enqueued) * 1e3
            print(f"\n[in-flight] {name}: delay {delay:.1f} ms, host gap {gap:.3f} ms, call {1e3 * (t_returned - t_call):.1f} ms")
            assert not ready, f"{name}: the stream had already drained before the call (delay {delay:.1f} ms, host gap {gap:.3f} ms)"
            assert delay >= 10.0 * gap, f"{name}: delay {delay:.1f} ms is not ten times the host gap {gap:.3f} ms"
            assert t_returned - t_call >= 0.5e-3 * delay, f"{name}: the call returned before the delay could have passed"
        return out, premise

    def close(self):
        try:
            hip.stream_synchronize(self.s)
        finally:
            self.a.free()
            self.b.free()
            hip.event_destroy(self.e0)
            hip.event_destroy(self.e1)
            hip.stream_destroy(self.s)


@pytest.fixture(scope="module")
def flight():
    f = Flight()
    try:
        f.calibrate()
        yield f
    finally:
        f.close()


class InFlight:
    """target: the buffer the library reads (holds the decoy); staged: the payload, uploaded synchronously."""

    def __init__(self, payload, decoy):
        payload, decoy = np.ascontiguousarray(payload), np.ascontiguousarray(decoy)
        assert payload.shape == decoy.shape and payload.dtype == decoy.dtype and payload.nbytes == decoy.nbytes
        if payload.dtype.kind == "f":
            assert np.isfinite(decoy).all()
        self.target = _lib.DeviceBuffer.from_numpy(decoy)
        self.staged = _lib.DeviceBuffer.from_numpy(payload)
        self.copy = (self.target.ptr, self.staged.ptr, payload.nbytes)

    def free(self):
        self.target.free()
        self.staged.free()


# ---- LAPs ---------------------------------------------------------------------------------------------------------------------

_ORACLE = {}


def _oracle(name, c, dtype, kind):
    key = (name, kind)
    if key not in _ORACLE:
        _ORACLE[key] = (jv_oracle_wide(c, np.float32, max_rounds=-1) if kind == "wide" else
                        jv_oracle(c, dtype, warm=True) if kind == "warm" else jv_oracle(c, dtype))
    return _ORACLE[key]


def _uniform(n, dtype, seed):
    c = np.random.default_rng(seed).random((n, n))
    return c.astype(np.float32) if dtype == np.float32 else c


LAP_CASES = {                        # name -> (dtype, cyto_lap_opts or None, the oracle's restatement)
    "cyto_lap_f32": (np.float32, None, "wide"),
    "cyto_lap_f32_opts mode=1": (np.float32, dict(mode=1), "chain"),
    "cyto_lap_f32_opts certify=1": (np.float32, dict(certify=1), "wide"),
    "cyto_lap_f64 cold": (np.float64, dict(mode=1), "chain"),
    "cyto_lap_f64 warm": (np.float64, None, "warm"),
}


@pytest.mark.parametrize("case", list(LAP_CASES))
def test_lap_reads_its_matrix_behind_the_callers_queue(flight, case):
    dtype, opts, kind = LAP_CASES[case]
    n = 1000
    tname = np.dtype(dtype).name
    payload, decoy = _uniform(n, dtype, 77), _uniform(n, dtype, 78)
    o, od = _oracle(f"payload_{tname}", payload, dtype, kind), _oracle(f"decoy_{tname}", decoy, dtype, kind)
    assert not np.array_equal(o["colsol"], od["colsol"]) and not np.array_equal(o["v"], od["v"])
    x = InFlight(payload, decoy)
    try:
        g, premise = flight.run(case, [x.copy], lambda s: lap_solve(None, dtype, return_info=True, device_ptr=x.target.ptr, n=n, ld=n,
                                                                   opts=opts, stream=s))
        premise()
        for k in ("rowsol", "colsol", "v", "u"):
            assert np.array_equal(g[k], o[k]), (case, k, "the decoy's" if np.array_equal(g[k], od[k]) else "a mixture")
        assert abs(g["total"] - o["total"]) <= (1e-9 if kind == "warm" else 1e-5) * max(1.0, abs(o["total"]))
        if opts and opts.get("certify"):
            h = lap_solve(payload, dtype, return_info=True, opts=opts)["info"]
            assert g["info"].certified == 1 and g["info"].gap_f64 == h.gap_f64 and g["info"].gap_rows == h.gap_rows
    finally:
        hip.stream_synchronize(flight.s)
        x.free()


@pytest.mark.parametrize("option", ["exact", "polish"])
def test_exact_and_polish_read_their_matrix_behind_the_callers_queue(flight, option):
    # instance 283 of the suite (n = 2 973, gap > 0: the repair / the polish really run).  Its optimum is certified unique, so the decoy
    # -- the same rows in reverse order -- has the reversed assignment as its one optimum: a different answer
    from tools import cross_unique
    payload = np.ascontiguousarray(cross_unique.instance("typed", 2973, 5283, 4), dtype=np.float32)
    decoy = np.ascontiguousarray(payload[::-1])
    n = len(payload)
    opts = {option: 1}
    h = lap_solve(payload, np.float32, return_info=True, opts=opts)              # the reference: NULL stream, host matrix
    assert h["info"].gap_f64 > 0.0 and (h["info"].exact_status == 2 if option == "exact" else h["info"].polished == 1)
    assert not np.array_equal(h["rowsol"][::-1], h["rowsol"])
    x = InFlight(payload, decoy)
    try:
        name = f"cyto_lap_f32_opts {option}=1"
        g, premise = flight.run(name, [x.copy], lambda s: lap_solve(None, np.float32, return_info=True, device_ptr=x.target.ptr, n=n,
                                                                   ld=n, opts=opts, stream=s))
        premise()
        for k in ("rowsol", "colsol", "u", "v"):
            assert np.array_equal(g[k], h[k]), (name, k)
        assert g["total"] == h["total"]
        for k in ("gap_f64", "gap_rows", "exact_status", "exact_edges", "exact_changed_rows", "polished"):
            assert getattr(g["info"], k) == getattr(h["info"], k), (name, k)
    finally:
        hip.stream_synchronize(flight.s)
        x.free()


def test_rowmap_reads_its_rows_behind_the_callers_queue(flight):
    rng = np.random.default_rng(79)
    nu, slots = 250, 4
    n = nu * slots
    rowmap = np.repeat(np.arange(nu), slots).astype(np.int32)
    payload = -(rng.random((nu, n)) ** 3).astype(np.float32)
    decoy = -(rng.random((nu, n)) ** 3).astype(np.float32)
    o, od = _oracle("rowmap_payload", payload[rowmap], np.float32, "wide"), _oracle("rowmap_decoy", decoy[rowmap], np.float32, "wide")
    assert not np.array_equal(o["colsol"], od["colsol"])
    x = InFlight(payload, decoy)
    try:
        g, premise = flight.run("cyto_lap_f32_rowmap", [x.copy],
                                lambda s: lap_solve_rows(None, rowmap, return_info=True, device_ptr=x.target.ptr, nu=nu, ld=n, stream=s))
        premise()
        for k in ("rowsol", "colsol", "v", "u"):
            assert np.array_equal(g[k], o[k]), k
    finally:
        hip.stream_synchronize(flight.s)
        x.free()


# ---- the cost build -----------------------------------------------------------------------------------------------------------

def _transform(tr, x, code, ptr, on_device, stream):
    """cyto_transform into a 0xFF-filled z; read back with plain cyto_memcpy_d2h right after the call."""
    G, C = x.shape
    Gpad, ldz = _up(G, 32), _up(C, 128)
    z = _lib.DeviceBuffer.from_numpy(np.full(Gpad * ldz * 4, 0xFF, np.uint8))
    try:
        _lib.check(_lib.lib().cyto_transform(tr, G, C, ptr, C, code, on_device, 0, z.ptr, ldz, Gpad, 0, stream))
        return z.to_numpy((Gpad, ldz), np.uint32)
    finally:
        if stream is not None:
            hip.stream_synchronize(stream)
        z.free()


@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("transform", ["standardize", "rank", "raw"])
def test_transform_reads_its_matrix_behind_the_callers_queue(flight, transform, dtype):
    tr = {"standardize": 0, "rank": 1, "raw": 2}[transform]
    dt, code = {"f32": (np.float32, 0), "u16": (np.uint16, 2)}[dtype]
    G, C = 1030, 1028
    rng = np.random.default_rng(80 + tr)
    payload, decoy = (rng.poisson(3.0, (G, C)) + (np.arange(G)[:, None] == np.arange(C)[None, :] % G)).astype(dt), None
    decoy = (rng.poisson(3.0, (G, C)) + (np.arange(G)[:, None] == (np.arange(C)[None, :] + 1) % G)).astype(dt)
    ref = _transform(tr, payload, code, payload.ctypes.data, 0, None)
    ref_decoy = _transform(tr, decoy, code, decoy.ctypes.data, 0, None)
    assert (ref[:G, :C] != ref_decoy[:G, :C]).mean() > 0.5
    x = InFlight(payload, decoy)
    try:
        name = f"cyto_transform {transform} {dtype}"
        got, premise = flight.run(name, [x.copy], lambda s: _transform(tr, payload, code, x.target.ptr, 1, s))
        premise()
        assert np.array_equal(got, ref), (name, f"{(got != ref).sum()} words differ; the decoy's: {np.array_equal(got, ref_decoy)}")
    finally:
        hip.stream_synchronize(flight.s)
        x.free()


METRICS = ["Pearson_correlation", "Spearman_correlation", "Euclidean"]


def _contract(metric, Gpad, S, C, zst, ldst, zsc, ldsc, stream):
    ldc = _up(C, 4)
    buf = _lib.DeviceBuffer.from_numpy(np.full((S, ldc), SENTINEL, np.float32))
    slots = np.ones(S, np.int64)
    ms = ctypes.c_double()
    try:
        _lib.check(_lib.lib().cyto_cost_metric(gcommon.METRICS[metric], Gpad, S, C, zst, ldst, zsc, ldsc, slots.ctypes.data, buf.ptr, ldc,
                                               ctypes.byref(ms), 0, stream))
        return buf.to_numpy((S, ldc), np.float32)
    finally:
        if stream is not None:
            hip.stream_synchronize(stream)
        buf.free()


@pytest.mark.parametrize("metric", METRICS)
def test_contraction_reads_both_operands_behind_the_callers_queue(flight, metric):
    rng = np.random.default_rng(90)
    G, S, C = 97, 130, 260

    def operand(ncols, depth):
        x = rng.poisson(depth * rng.lognormal(0.0, 1.0, (G, 1)) * np.ones((1, ncols))).astype(np.float32)
        x[rng.integers(G, size=ncols), np.arange(ncols)] += 1
        x[rng.integers(G, size=ncols), np.arange(ncols)] += 2
        z = gcommon.StandardizedMatrix(x, False, 0, metric)
        host = z.buf.to_numpy((z.Gpad, z.ld), np.float32)
        z.buf.free()
        return types.SimpleNamespace(host=host, Gpad=z.Gpad, ld=z.ld)

    sc, st, sc_decoy, st_decoy = operand(C, 0.5), operand(S, 3.0), operand(C, 0.5), operand(S, 3.0)
    xsc, xst = InFlight(sc.host, sc_decoy.host), InFlight(st.host, st_decoy.host)
    try:
        ref = _contract(metric, sc.Gpad, S, C, xst.staged.ptr, st.ld, xsc.staged.ptr, sc.ld, None)
        ref_decoy = _contract(metric, sc.Gpad, S, C, xst.target.ptr, st.ld, xsc.target.ptr, sc.ld, None)
        assert np.isfinite(ref[:, :C]).all() and (ref[:, :C] != ref_decoy[:, :C]).mean() > 0.5
        name = f"cyto_cost_metric {metric}"
        got, premise = flight.run(name, [xsc.copy, xst.copy],
                                  lambda s: _contract(metric, sc.Gpad, S, C, xst.target.ptr, st.ld, xsc.target.ptr, sc.ld, s))
        premise()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, f"{(got.view(np.uint32) != ref.view(np.uint32)).sum()} words differ")
    finally:
        hip.stream_synchronize(flight.s)
        xsc.free()
        xst.free()


def test_csc_to_dense_on_the_callers_stream(flight):
    # host inputs: nothing is in flight, only the output is checked -- read with cyto_memcpy_d2h right after the call
    import scipy.sparse as sp
    rng = np.random.default_rng(91)
    G, C = 700, 333
    m = sp.random(G, C, density=0.05, format="csc", random_state=np.random.RandomState(5), data_rvs=lambda k: rng.integers(1, 50, k).astype(np.float64))
    m.sum_duplicates()
    vals = np.ascontiguousarray(m.data, dtype=np.float32)
    colptr, rowidx = np.ascontiguousarray(m.indptr, dtype=np.int64), np.ascontiguousarray(m.indices, dtype=np.int32)
    ld = _up(C, 4)
    buf = _lib.DeviceBuffer.from_numpy(np.full((G, ld), SENTINEL, np.float32))
    try:
        _lib.check(_lib.lib().cyto_csc_to_dense_f32(G, C, len(vals), colptr.ctypes.data, rowidx.ctypes.data, vals.ctypes.data, buf.ptr, ld,
                                                   0, flight.s))
        got = buf.to_numpy((G, ld), np.float32)
        assert np.array_equal(got[:, :C], m.toarray().astype(np.float32)) and not got[:, C:].any()
    finally:
        hip.stream_synchronize(flight.s)
        buf.free()


# ---- views of a resident table (cyto_select, cyto_value_range) ---------------------------------------------------------------

VIEW_G, VIEW_C = 700, 333


def _view_tables():
    """(payload, decoy): float64 tables of one shape; the decoy is finite, holds other values everywhere and has another range."""
    rng = np.random.default_rng(92)
    payload = rng.poisson(3.0, (VIEW_G, VIEW_C)).astype(np.float64)
    payload[rng.integers(0, VIEW_G, 50), rng.integers(0, VIEW_C, 50)] = 0.5          # not integral
    payload[rng.integers(0, VIEW_G, 30), rng.integers(0, VIEW_C, 30)] = 0.1          # ... and no float32 value
    payload[VIEW_G - 1, VIEW_C - 1], payload[0, 0] = 60000.0, -2.0
    decoy = rng.integers(1000, 2000, (VIEW_G, VIEW_C)).astype(np.float64)
    assert (payload != decoy).all()
    return payload, decoy


def _view_lists():
    rng = np.random.default_rng(93)
    rows = np.ascontiguousarray(np.r_[rng.integers(0, VIEW_G, 400), VIEW_G - 1, 0].astype(np.int64))
    cols = np.ascontiguousarray(np.r_[VIEW_C - 1, rng.integers(0, VIEW_C, 200), 0].astype(np.int64))
    return [(None, None), (rows, cols)]          # (without lists first: nothing but the table is in flight then)


@pytest.mark.parametrize("dst", ["float32", "uint16"])
def test_select_reads_its_table_behind_the_callers_queue(flight, dst):
    from test_resident_select_gpu import DST, SRC, expect
    payload, decoy = _view_tables()
    x = InFlight(payload, decoy)
    try:
        for rows, cols in _view_lists():
            Gs, Cs = (VIEW_G if rows is None else len(rows)), (VIEW_C if cols is None else len(cols))
            ix = np.ix_(np.arange(VIEW_G) if rows is None else rows, np.arange(VIEW_C) if cols is None else cols)
            want, ok, defined = expect(payload[ix], dst)
            want_decoy, _, _ = expect(decoy[ix], dst)
            assert defined.mean() > 0.9 and (want[defined] != want_decoy[defined]).all()
            ld_dst = Cs + 3
            out = _lib.DeviceBuffer.from_numpy(np.full(Gs * ld_dst * np.dtype(DST[dst][0]).itemsize, 0xA5, np.uint8))
            bad = ctypes.c_int64(-7)

            def call(s):
                st = _lib.lib().cyto_select(VIEW_G, VIEW_C, x.target.ptr, VIEW_C, SRC["float64"][1], None if rows is None else rows.ctypes.data, Gs,
                                            None if cols is None else cols.ctypes.data, Cs, out.ptr, ld_dst, DST[dst][1], ctypes.byref(bad), 0, s)
                return st, out.to_numpy((Gs, ld_dst), DST[dst][0])             # (plain cyto_memcpy_d2h, at once)

            name = f"cyto_select float64 -> {dst}" + ("" if rows is None else " with lists")
            try:
                (st, got), premise = flight.run(name, [x.copy], call)
                premise()
                assert st == 0
                block = got[:, :Cs]
                n_decoy = int((block[defined] == want_decoy[defined]).sum())
                assert np.array_equal(block[defined].view(np.uint8), want[defined].view(np.uint8)), \
                    (name, f"{(block[defined] != want[defined]).sum()} elements are not the payload's; {n_decoy} are the decoy's")
                assert bad.value == int(np.count_nonzero(~ok)), (name, bad.value)
                assert (np.ascontiguousarray(got[:, Cs:]).view(np.uint8) == 0xA5).all(), (name, "padding written")
            finally:
                hip.stream_synchronize(flight.s)
                out.free()
            _lib.check(_lib.lib().cyto_memcpy_h2d(x.target.ptr, decoy.ctypes.data, decoy.nbytes, 0))      # (the next round starts from the decoy)
    finally:
        hip.stream_synchronize(flight.s)
        x.free()


def test_value_range_reads_its_table_behind_the_callers_queue(flight):
    from test_resident_select_gpu import SRC, expect_range
    payload, decoy = _view_tables()
    x = InFlight(payload, decoy)
    try:
        for rows, cols in _view_lists():
            Gs, Cs = (VIEW_G if rows is None else len(rows)), (VIEW_C if cols is None else len(cols))
            ix = np.ix_(np.arange(VIEW_G) if rows is None else rows, np.arange(VIEW_C) if cols is None else cols)
            want, want_decoy = expect_range(payload[ix]), expect_range(decoy[ix])
            assert all(want[k] != want_decoy[k] for k in ("lo", "hi", "non_integral", "not_f32_exact"))

            def call(s):
                lo, hi = ctypes.c_double(), ctypes.c_double()
                ilo, ihi, nint, nfin, n32 = (ctypes.c_int64(-7) for _ in range(5))
                st = _lib.lib().cyto_value_range(VIEW_G, VIEW_C, x.target.ptr, VIEW_C, SRC["float64"][1], None if rows is None else rows.ctypes.data,
                                                 Gs, None if cols is None else cols.ctypes.data, Cs, ctypes.byref(lo), ctypes.byref(hi),
                                                 ctypes.byref(ilo), ctypes.byref(ihi), ctypes.byref(nint), ctypes.byref(nfin), ctypes.byref(n32), 0, s)
                return st, dict(lo=lo.value, hi=hi.value, ilo=ilo.value, ihi=ihi.value, non_integral=nint.value, non_finite=nfin.value,
                                not_f32_exact=n32.value)

            name = "cyto_value_range float64" + ("" if rows is None else " with lists")
            try:
                (st, got), premise = flight.run(name, [x.copy], call)
                premise()
                assert st == 0
                assert got == want, (name, got, "the decoy's" if got == want_decoy else "neither")
            finally:
                hip.stream_synchronize(flight.s)
            _lib.check(_lib.lib().cyto_memcpy_h2d(x.target.ptr, decoy.ctypes.data, decoy.nbytes, 0))      # (the next round starts from the decoy)
    finally:
        hip.stream_synchronize(flight.s)
        x.free()
