"""cyto_assign_metric_ex with on_device = 1 matrices at the C ABI (csrc/cost.hip: assign_metric_impl), which no other module calls
with a pitch above the width or a base inside an allocation -- above all the block pipeline (C > 16 384), where a device scRNA
matrix is transformed block by block where it lies, at sc + c0 * element size with the caller's pitch.

Every case is judged on the float64 cost, oracle.precision.cost(metric, sc, st): the assignment's total on it against the optimum
(scipy's, small case) or a dual lower bound (block pipeline), within 2 C eps of the documented tolerance (TOL and _eps of
tests/test_cost_precision_gpu.py); the slot counts exactly.  Then the header's claim: mapped_spot and total_cost are, bit for bit,
those of the same call with host matrices.  Every element of a device buffer that is not data is a poison (tests/_layouts.py), and
the buffers are byte-identical afterwards."""
import ctypes

import numpy as np
import pytest

import _layouts as LY
from cytospace_amd import _lib
from cytospace_amd import common as gcommon
from cytospace_amd.lap import lap_solve_rows
from oracle import precision as P
from test_cost_precision_gpu import TOL, _eps, _lsap_optimum
from test_device_inputs_gpu import Resident
from tools import instances

pytestmark = pytest.mark.gpu

METRICS = ["Pearson_correlation", "Spearman_correlation", "Euclidean"]
CODE = {np.dtype(np.float32): _lib.CYTO_DTYPE_F32, np.dtype(np.float64): _lib.CYTO_DTYPE_F64, np.dtype(np.uint16): _lib.CYTO_DTYPE_U16,
        np.dtype(np.uint8): _lib.CYTO_DTYPE_U8}
BAD_ARG = 1
PIPELINE_ABOVE = 16384               # cost.hip: metric != Euclidean && C > 2 * WBLK (WBLK = 8192) takes the block pipeline


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    yield
    _SMALL.clear()                   # (the block pipeline's float64 costs are 215 MB each)
    _BIG.clear()


def takes_block_pipeline(metric, C):
    return metric != "Euclidean" and C > PIPELINE_ABOVE


def _matrix(data, ld, dtype, on_device):
    m = _lib.Matrix()
    m.data, m.ld, m.is_f64, m.on_device = data, ld, CODE[np.dtype(dtype)], on_device
    return m


def host_matrix(x):
    assert x.flags.c_contiguous
    return _matrix(x.ctypes.data, x.shape[1], x.dtype, 0)


def device_matrix(r):
    return _matrix(r.ptr, r.ld, r.host.dtype, 1)


def assign(metric, G, C, S, msc, mst, slots):
    """(status, mapped_spot, total_cost) of cyto_assign_metric_ex."""
    mapped = np.full(C, -1, np.int64)
    total = ctypes.c_double(np.nan)
    info = _lib.AssignInfo()
    st = _lib.lib().cyto_assign_metric_ex(gcommon.METRICS[metric], G, ctypes.byref(msc), C, ctypes.byref(mst), S, slots.ctypes.data, 0,
                                          mapped.ctypes.data, ctypes.byref(total), ctypes.byref(info), 0)
    return st, mapped, total.value


def same_bits(a, b):
    return np.array_equal(np.array([a], np.float64).view(np.uint64), np.array([b], np.float64).view(np.uint64))


# ---- (a) the small case ---------------------------------------------------------------------------------------------------------

SMALL = (97, 257, 60, 7)
SMALL_LAYOUTS = ("tight", "odd_pitch", "offset_base", "quad_offset_base", "wide")
_SMALL = {}


def small_instance():
    if "x" not in _SMALL:
        G, C, S, seed = SMALL
        sc, st, slots = instances.synth_expression(G, C, S, seed=seed)
        assert slots.sum() == C and sc.max() <= 255 and st.max() <= 65535 and sc.std(0).min() > 0 and st.std(0).min() > 0
        _SMALL["x"] = (sc, st, np.ascontiguousarray(slots, dtype=np.int64))
    return _SMALL["x"]


def small_reference(metric):
    if metric not in _SMALL:
        sc, st, slots = small_instance()
        ref = P.cost(metric, sc, st)
        _SMALL[metric] = (ref, _lsap_optimum(ref, slots))
    return _SMALL[metric]


@pytest.mark.parametrize("st_type", [np.uint16, np.float64], ids=lambda d: "st_" + np.dtype(d).name)
@pytest.mark.parametrize("sc_type", [np.uint8, np.float32], ids=lambda d: "sc_" + np.dtype(d).name)
@pytest.mark.parametrize("metric", METRICS)
def test_small_case_in_every_placement_and_layout(metric, sc_type, st_type):
    G, C, S, _ = SMALL
    sc32, st32, slots = small_instance()
    sc, st = np.ascontiguousarray(sc32.astype(sc_type)), np.ascontiguousarray(st32.astype(st_type))
    assert np.array_equal(sc, sc32) and np.array_equal(st, st32)
    ref, best = small_reference(metric)
    eps = _eps(metric, ref)
    assert not takes_block_pipeline(metric, C)
    status, h_mapped, h_total = assign(metric, G, C, S, host_matrix(sc), host_matrix(st), slots)
    assert status == 0
    fails, worst = [], -np.inf
    for layout in SMALL_LAYOUTS:
        with Resident(sc, layout, 4, np.nan) as rsc, Resident(st, layout, 4, np.nan) as rst:
            for place, msc, mst in (("both on the device", device_matrix(rsc), device_matrix(rst)),
                                    ("scRNA on the device", device_matrix(rsc), host_matrix(st)),
                                    ("ST on the device", host_matrix(sc), device_matrix(rst))):
                tag = f"{metric} {sc.dtype.name}/{st.dtype.name} {layout} (ld {rsc.ld} / {rst.ld}), {place}"
                status, mapped, total = assign(metric, G, C, S, msc, mst, slots)
                if status != 0:
                    fails.append(f"{tag}: status {status}")
                    continue
                if mapped.min() < 0 or mapped.max() >= S or not np.array_equal(np.bincount(mapped, minlength=S), slots):
                    fails.append(f"{tag}: the slot counts are not the instance's")
                    continue
                mine = float(ref[mapped, np.arange(C)].sum())
                worst = max(worst, mine - best)
                if not best - 1e-9 * abs(best) <= mine <= best + 2 * C * eps:
                    fails.append(f"{tag}: total {mine!r} on the float64 cost, optimum {best!r}, bound 2 C eps = {2 * C * eps:.3g}")
                if not np.array_equal(mapped, h_mapped) or not same_bits(total, h_total):
                    fails.append(f"{tag}: {(mapped != h_mapped).sum()} cells mapped differently than with host matrices, "
                                 f"total {total!r} against {h_total!r}")
            if not (rsc.untouched() and rst.untouched()):
                fails.append(f"{metric} {layout}: a caller's buffer changed")
    print(f"\n[device assign, small] {metric} {sc.dtype.name}/{st.dtype.name}: at most {worst:.3g} above the optimum "
          f"(2 C eps = {2 * C * eps:.3g})")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:20])


# ---- (b) the block pipeline ------------------------------------------------------------------------------------------------------

BIG = (240, 16385, 1640, 41)
_BIG = {}


def big_instance():
    if "x" not in _BIG:
        G, C, S, seed = BIG
        sc, st, slots = instances.synth_expression(G, C, S, seed=seed)
        assert slots.sum() == C and sc.max() <= 255 and st.max() <= 65535 and sc.std(0).min() > 0 and st.std(0).min() > 0
        _BIG["x"] = (sc, st, np.ascontiguousarray(slots, dtype=np.int64))
    return _BIG["x"]


def big_reference(metric):
    """(the float64 cost, a lower bound on its optimum from the device solver's duals on the rounded cost: any duals give a valid
    bound, so nothing here depends on that solver being right)."""
    if metric not in _BIG:
        sc, st, slots = big_instance()
        ref = P.cost(metric, sc, st)
        assert np.isfinite(ref).all()
        loc = np.repeat(np.arange(len(slots)), slots)
        g = lap_solve_rows(ref.astype(np.float32), loc)
        _BIG[metric] = (ref, P.dual_lower_bound(ref, loc, g["u"], g["v"]))
    return _BIG[metric]


SC_CASES = {"uint8 odd_pitch": (np.uint8, "odd_pitch"), "float32 offset_base": (np.float32, "offset_base")}


@pytest.mark.parametrize("sc_case", list(SC_CASES))
@pytest.mark.parametrize("metric", ["Pearson_correlation", "Spearman_correlation"])
def test_block_pipeline_with_a_device_scrna_matrix(metric, sc_case):
    """C = 16 385 is the smallest extent that takes the pipeline: blocks of 2 048, 8 192 and 6 145 columns, the last of them odd (the
    one-column transform kernels).  uint8 with an odd pitch; float32 with a base that is not an allocation's start."""
    G, C, S, _ = BIG
    sc32, st32, slots = big_instance()
    sc_type, layout = SC_CASES[sc_case]
    sc, st = np.ascontiguousarray(sc32.astype(sc_type)), np.ascontiguousarray(st32.astype(np.uint16))
    assert np.array_equal(sc, sc32) and np.array_equal(st, st32) and takes_block_pipeline(metric, C)
    ref, lb = big_reference(metric)
    status, h_mapped, h_total = assign(metric, G, C, S, host_matrix(sc), host_matrix(st), slots)
    assert status == 0
    fails = []
    with Resident(sc, layout, 4, np.nan) as rsc, Resident(st, "odd_pitch", 4, np.nan) as rst:
        assert rsc.ld > C and (layout != "offset_base" or rsc.ptr != rsc.buf.ptr)
        for place, mst in (("ST on the device", device_matrix(rst)), ("ST on the host", host_matrix(st))):
            tag = f"{metric} scRNA {sc_case} (ld {rsc.ld}), {place}"
            status, mapped, total = assign(metric, G, C, S, device_matrix(rsc), mst, slots)
            if status != 0:
                fails.append(f"{tag}: status {status}")
                continue
            if mapped.min() < 0 or mapped.max() >= S or not np.array_equal(np.bincount(mapped, minlength=S), slots):
                fails.append(f"{tag}: the slot counts are not the instance's")
                continue
            mine = float(ref[mapped, np.arange(C)].sum())
            print(f"\n[device assign, block pipeline] {tag}: {mine - lb:.3g} above the dual bound (2 C eps = {2 * C * TOL:.3g})")
            if not mine <= lb + 2 * C * TOL:
                fails.append(f"{tag}: total {mine!r} on the float64 cost, dual bound {lb!r}, 2 C eps = {2 * C * TOL:.3g}")
            if not np.array_equal(mapped, h_mapped) or not same_bits(total, h_total):
                fails.append(f"{tag}: {(mapped != h_mapped).sum()} cells mapped differently than with host matrices, "
                             f"total {total!r} against {h_total!r}")
        if not (rsc.untouched() and rst.untouched()):
            fails.append(f"{metric} {sc_case}: a caller's buffer changed")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:20])


def test_euclidean_at_the_same_extent_is_the_split_path():
    """The documented gate (cost.hip: metric != Euclidean && C > 16 384) keeps Euclidean on the whole-matrix transform, whose device
    form takes the caller's pitch through cyto_transform: the same bits as with host matrices there too."""
    G, C, S, _ = BIG
    sc32, st32, slots = big_instance()
    sc, st = np.ascontiguousarray(sc32.astype(np.uint8)), np.ascontiguousarray(st32.astype(np.uint16))
    assert not takes_block_pipeline("Euclidean", C) and takes_block_pipeline("Pearson_correlation", C) and C == PIPELINE_ABOVE + 1
    status, h_mapped, h_total = assign("Euclidean", G, C, S, host_matrix(sc), host_matrix(st), slots)
    assert status == 0 and np.array_equal(np.bincount(h_mapped, minlength=S), slots)
    with Resident(sc, "odd_pitch", 4, np.nan) as rsc, Resident(st, "odd_pitch", 4, np.nan) as rst:
        status, mapped, total = assign("Euclidean", G, C, S, device_matrix(rsc), device_matrix(rst), slots)
        assert status == 0
        assert np.array_equal(mapped, h_mapped) and same_bits(total, h_total), ((mapped != h_mapped).sum(), total, h_total)
        assert rsc.untouched() and rst.untouched()


# ---- (c) refusals --------------------------------------------------------------------------------------------------------------

def test_refusals():
    G, C, S, _ = SMALL
    sc32, st32, slots = small_instance()
    sc, st = np.ascontiguousarray(sc32.astype(np.uint8)), np.ascontiguousarray(st32.astype(np.uint16))
    with Resident(sc, "odd_pitch", 4, np.nan) as rsc, Resident(st, "odd_pitch", 4, np.nan) as rst:
        good_sc, good_st = device_matrix(rsc), device_matrix(rst)
        cases = {
            "device scRNA with ld < C": (_matrix(rsc.ptr, C - 1, np.uint8, 1), good_st),
            "device ST with ld < S": (good_sc, _matrix(rst.ptr, S - 1, np.uint16, 1)),
            "host scRNA with ld != C": (_matrix(sc.ctypes.data, C + 1, np.uint8, 0), good_st),
            "host ST with ld != S": (good_sc, _matrix(st.ctypes.data, S + 1, np.uint16, 0)),
            "host ST with ld < S": (good_sc, _matrix(st.ctypes.data, S - 1, np.uint16, 0)),
            "null scRNA on the device": (_matrix(None, rsc.ld, np.uint8, 1), good_st),
            "null ST on the device": (good_sc, _matrix(None, rst.ld, np.uint16, 1)),
            "null scRNA on the host": (_matrix(None, C, np.uint8, 0), good_st),
        }
        for name, (msc, mst) in cases.items():
            status, mapped, total = assign("Pearson_correlation", G, C, S, msc, mst, slots)
            assert status == BAD_ARG, (name, status)
            assert (mapped == -1).all() and np.isnan(total), name
        status, mapped, _ = assign("Pearson_correlation", G, C, S, good_sc, good_st, slots)      # the control
        assert status == 0 and np.array_equal(np.bincount(mapped, minlength=S), slots)
