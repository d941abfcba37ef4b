"""The first row caches from the column reduction's own pass (colred_partial_append, fused_w / fused_theta / fused_fixup, the row-list
form of build_row_caches_wave) against the wide restatement, bit for bit -- results and semantic counters do not depend
on who built a cache, so every solve must equal oracle.jv.jv_oracle_wide whichever rows the lists certified.

The knob that moves the gate down to 2 048 rows (CYTO_CACHE_FUSED) is read once per process, so every case runs in a child
interpreter; the child solves, compares and reports how far cyto_fused_cache_solves() and cyto_fused_cache_fallback_rows() moved
per solve.  The numpy model of the kernels: tests/test_cache_fused_cpu.py (its overflow matrix is used here too)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r'''
import json, sys
import numpy as np
from cytospace_amd import _lib
from cytospace_amd.lap import lap_solve, lap_solve_batch
from oracle.jv import jv_oracle_wide
import _layouts as LY
from test_cache_fused_cpu import overflow_cost

# (tests/test_lap_gpu.py: WIDE_KEYS -- the semantic counters of the wide solver and their names in the restatement)
WIDE_KEYS = [("scans_redtransfer", "scans_redtransfer"), ("scans_arr", "scans_arr"), ("scans_aug_init", "scans_aug_init"),
             ("scans_aug_relax", "scans_aug_relax"), ("augmentations", "augmentations"), ("path_hops", "path_hops"),
             ("free_after_colred", "free_after_colred"), ("free_after_arr2", "free_after_arr"), ("wide_rounds", "arr_rounds"),
             ("wide_retired", "arr_retired"), ("wide_scaled", "arr_scaled"), ("wide_phases", "arr_phases")]
ROUNDS = (0, 2)


def few_types(n):
    # the generator of tests/test_wide_embedded_gpu.py (few cell types: the sampled column minima lie far above the final ones)
    rng = np.random.default_rng(5)
    types = 6
    prof = rng.normal(size=(types, 64)).astype(np.float32)
    rows = prof[rng.integers(0, types, n)] + 0.05 * rng.normal(size=(n, 64)).astype(np.float32)
    cols = prof[rng.integers(0, types, n)] + 0.05 * rng.normal(size=(n, 64)).astype(np.float32)
    return -(rows @ cols.T).astype(np.float32)


def instance(case):
    rng = np.random.default_rng(42)
    if case.startswith("uniform"):
        n = int(case[7:])
        return rng.random((n, n)).astype(np.float32)
    if case == "pitched2051":
        return rng.random((2051, 2051)).astype(np.float32)
    if case == "ties2100":
        return rng.integers(0, 10, (2100, 2100)).astype(np.float32)
    if case == "repeated2200":
        return np.repeat(rng.random((550, 2200)), 4, axis=0).astype(np.float32)
    if case == "few_types2400":
        return few_types(2400)
    if case == "overflow2304":
        return overflow_cost(2304)
    raise SystemExit("unknown case " + case)


def compare(g, o, what):
    for k in ("rowsol", "colsol", "u", "v"):
        assert np.array_equal(g[k], o[k]), (what, k)
    od, gd = o["stats"].as_dict(), g["info"].as_dict()
    assert gd["wide"] == 1
    for kg, ko in WIDE_KEYS:
        assert gd[kg] == od[ko], (what, kg, gd[kg], od[ko])


def main():
    case = sys.argv[1]
    fused, fallback, reads = [], [], []
    if case == "batch2300":
        # two problems in one call: the lists are for one problem per call
        rng = np.random.default_rng(42)
        cs = [rng.random((2300, 2300)).astype(np.float32) for _ in range(2)]
        before = _lib.fused_cache_solves()
        for r in ROUNDS:
            res = lap_solve_batch(cs, return_info=True, opts=dict(mode=2, wide_rounds=r))
            for c, g in zip(cs, res):
                compare(g, jv_oracle_wide(c, np.float32, max_rounds=-1 if r == 0 else r), (case, r))
        print(json.dumps({"n": 2300, "solves": 2 * len(ROUNDS), "fused": [_lib.fused_cache_solves() - before], "fallback": [], "reads": []}))
        return
    c = instance(case)
    n = c.shape[0]
    dev = None
    if case == "pitched2051":
        # pitch 2 112, NaN in every element that is not data (the padding of each row, the tail of the buffer)
        ld = 2112
        host = np.full(n * ld + LY.TAIL, LY.poison_value(np.float32, float("nan")), np.float32)
        host[:n * ld].reshape(n, ld)[:, :n] = c
        assert np.array_equal(LY.extract(host, 0, ld, n, n), c) and np.isnan(host[:n * ld].reshape(n, ld)[:, n:]).all()
        dev = _lib.DeviceBuffer.from_numpy(host)
    for r in ROUNDS:
        o = jv_oracle_wide(c, np.float32, max_rounds=-1 if r == 0 else r)
        b0, f0 = _lib.fused_cache_solves(), _lib.fused_cache_fallback_rows()
        if dev is not None:
            g = lap_solve(None, np.float32, return_info=True, device_ptr=dev.ptr, n=n, ld=2112, opts=dict(mode=2, wide_rounds=r))
        else:
            g = lap_solve(c, np.float32, return_info=True, opts=dict(mode=2, wide_rounds=r))
        compare(g, o, (case, r))
        fused.append(_lib.fused_cache_solves() - b0)
        fallback.append(_lib.fused_cache_fallback_rows() - f0)
        reads.append(int(g["info"].hbm_row_reads))
    if dev is not None:
        dev.free()
    print(json.dumps({"n": n, "solves": len(ROUNDS), "fused": fused, "fallback": fallback, "reads": reads}))


main()
'''


def _run(tmp_path, case, knob):
    script = tmp_path / "fused_worker.py"
    script.write_text(_WORKER)
    env = {k: v for k, v in os.environ.items() if k != "CYTO_CACHE_FUSED"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    if knob is not None:
        env["CYTO_CACHE_FUSED"] = str(knob)
    r = subprocess.run([sys.executable, str(script), case], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, knob, out)
    return out


@pytest.mark.parametrize("n", [2051, 2300, 4100])
def test_fused_uniform(tmp_path, n):
    # 2 051: a ragged last quad, barely more columns than fused_theta reads; 4 100: more than one block of rows per column block
    out = _run(tmp_path, f"uniform{n}", 2)
    assert out["fused"] == [1] * out["solves"]
    assert all(f <= n // 8 for f in out["fallback"])


def test_fused_pitched_rows_with_nan_padding(tmp_path):
    out = _run(tmp_path, "pitched2051", 2)
    assert out["fused"] == [1] * out["solves"]
    assert all(f <= 2051 // 8 for f in out["fallback"])


def test_fused_integer_ties_fall_back_on_every_row(tmp_path):
    # integer costs 0 ... 9: no list certifies its row; the full builder runs as if there had been no lists
    out = _run(tmp_path, "ties2100", 2)
    assert out["fused"] == [1] * out["solves"] and out["fallback"] == [2100] * out["solves"]


def test_fused_repeated_rows(tmp_path):
    # 550 distinct rows x 4: the copies are skipped by the fix-up and replicated afterwards
    out = _run(tmp_path, "repeated2200", 2)
    assert out["fused"] == [1] * out["solves"]
    assert all(f <= 550 for f in out["fallback"])       # (only the first row of a run can go on the row list)


def test_fused_few_cell_types_give_the_lists_up(tmp_path):
    # more than n / 8 rows fail: every row is built by the row builder
    out = _run(tmp_path, "few_types2400", 2)
    assert out["fused"] == [1] * out["solves"] and out["fallback"] == [2400] * out["solves"]


def test_fused_overflowing_lists_go_to_the_row_list(tmp_path):
    # every 16th row lists more than 512 columns: those rows, and only a few others, are built from the row list
    out = _run(tmp_path, "overflow2304", 2)
    assert out["fused"] == [1] * out["solves"]
    assert all(2304 // 16 <= f <= 2304 // 8 for f in out["fallback"])


def test_fused_not_for_two_problems_in_one_call(tmp_path):
    out = _run(tmp_path, "batch2300", 2)
    assert out["fused"] == [0]


@pytest.mark.parametrize("knob", [0, None])
def test_fused_off_below_the_default_gate(tmp_path, knob):
    # 0: never; unset: from 32 768 rows on
    out = _run(tmp_path, "uniform2300", knob)
    assert out["fused"] == [0] * out["solves"] and out["fallback"] == [0] * out["solves"]
