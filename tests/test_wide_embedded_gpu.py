"""The embedded form of the wide solver's searches (wide_aug<.., EMB>: several searches of one problem at once, prices in global memory,
every cache entry carried less its column's price and repaired by the commits) against the wide restatement, bit for bit.

The knobs that select the form (CYTO_AUG_LDS, CYTO_AUG_EMBED) are read once per process, so every case runs in a child interpreter;
the child solves, compares with oracle.jv.jv_oracle_wide and reports how far cyto_wide_embedded_solves() moved."""
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
from cytospace_amd.lap import lap_solve
from oracle.jv import jv_oracle_wide

# (tests/test_lap_gpu.py: WIDE_KEYS -- the semantic counters of the wide solver and their names in the restatement)
WIDE_KEYS = [("scans_redtransfer", "scans_redtransfer"), ("scans_arr", "scans_arr"), ("scans_aug_init", "scans_aug_init"),
             ("scans_aug_relax", "scans_aug_relax"), ("augmentations", "augmentations"), ("path_hops", "path_hops"),
             ("free_after_colred", "free_after_colred"), ("free_after_arr2", "free_after_arr"), ("wide_rounds", "arr_rounds"),
             ("wide_retired", "arr_retired"), ("wide_scaled", "arr_scaled"), ("wide_phases", "arr_phases")]


def few_types(n):
    # the generator of tests/test_lap_gpu.py::test_wide_full_row_fallbacks_on_near_equal_columns
    rng = np.random.default_rng(5)
    types = 6
    prof = rng.normal(size=(types, 64)).astype(np.float32)
    rows = prof[rng.integers(0, types, n)] + 0.05 * rng.normal(size=(n, 64)).astype(np.float32)
    cols = prof[rng.integers(0, types, n)] + 0.05 * rng.normal(size=(n, 64)).astype(np.float32)
    return -(rows @ cols.T).astype(np.float32)


def instances(case):
    rng = np.random.default_rng(42)
    if case == "uniform":
        return [rng.random((2300, 2300)).astype(np.float32)]
    if case == "uniform700":
        return [rng.random((700, 700)).astype(np.float32)]
    if case == "tiny":
        return [rng.random((n, n)).astype(np.float32) for n in (3, 64, 65)]
    if case == "ties":
        return [rng.integers(0, 10, (400, 400)).astype(np.float32)]
    if case == "repeated":
        return [np.repeat(rng.random((150, 600)), 4, axis=0).astype(np.float32)]
    if case == "few_types":
        return [few_types(1200)]
    raise SystemExit("unknown case " + case)


def main():
    case, pars, rounds = sys.argv[1], json.loads(sys.argv[2]), json.loads(sys.argv[3])
    solves, dense_aug, searches = 0, [], []
    before = _lib.wide_embedded_solves()
    for c in instances(case):
        ref = {}
        for r in rounds:
            ref[r] = jv_oracle_wide(c, np.float32, max_rounds=-1 if r == 0 else max(r, 0))      # once per instance and round cap
        for par in pars:
            for r in rounds:
                o = ref[r]
                g = lap_solve(c, np.float32, return_info=True, opts=dict(mode=2, wide_rounds=r, wide_par=par))
                for k in ("rowsol", "colsol", "u", "v"):
                    assert np.array_equal(g[k], o[k]), (case, c.shape, par, r, k)
                od, gd = o["stats"].as_dict(), g["info"].as_dict()
                assert gd["wide"] == 1
                for kg, ko in WIDE_KEYS:
                    assert gd[kg] == od[ko], (case, c.shape, par, r, kg, gd[kg], od[ko])
                solves += 1
                dense_aug.append(int(gd["wide_dense_aug"]))
                searches.append(int(gd["augmentations"]))
    print(json.dumps({"solves": solves, "embedded": _lib.wide_embedded_solves() - before, "dense_aug": dense_aug, "searches": searches}))


main()
'''


def _run(tmp_path, case, pars, rounds, lds, embed):
    script = tmp_path / "embedded_worker.py"
    script.write_text(_WORKER)
    env = {k: v for k, v in os.environ.items() if k not in ("CYTO_AUG_LDS", "CYTO_AUG_EMBED")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    if lds is not None:
        env["CYTO_AUG_LDS"] = str(lds)
    if embed is not None:
        env["CYTO_AUG_EMBED"] = str(embed)
    r = subprocess.run([sys.executable, str(script), case, json.dumps(pars), json.dumps(rounds)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, pars, rounds, lds, embed, out)
    return out


@pytest.mark.parametrize("par", [2, 16])
def test_embedded_uniform(tmp_path, par):
    # wide_rounds = -1 leaves about n searches: every entry of cache_red is repaired many times
    out = _run(tmp_path, "uniform", [par], [0, 2, -1], lds=1, embed=2)
    assert out["solves"] == 3 and out["embedded"] == 3
    assert out["searches"][2] > 2300 // 5          # (the column reduction of a uniform instance leaves about n / e rows free)


def test_embedded_never_when_switched_off(tmp_path):
    out = _run(tmp_path, "uniform", [16], [2], lds=1, embed=0)
    assert out["solves"] == 1 and out["embedded"] == 0


def test_embedded_uniform_owners_global(tmp_path):
    # neither prices nor owners in LDS: the CLDS = false instantiation
    out = _run(tmp_path, "uniform700", [2, 16], [0, 2, -1], lds=0, embed=2)
    assert out["solves"] == 6 and out["embedded"] == 6


def test_embedded_tiny_and_unpadded(tmp_path):
    # unused cache slots (n < 64), n not a multiple of 64
    out = _run(tmp_path, "tiny", [2], [0, -1], lds=1, embed=2)
    assert out["solves"] == 6 and out["embedded"] == 6


def test_embedded_ties(tmp_path):
    # integer costs 0 ... 9: most searches of a batch collide; the discarded ones must leave cache_red alone
    out = _run(tmp_path, "ties", [16], [0, -1], lds=1, embed=2)
    assert out["solves"] == 2 and out["embedded"] == 2


def test_embedded_repeated_rows(tmp_path):
    # 150 distinct rows x 4: the replicated caches each have their own entries in the inverse index
    out = _run(tmp_path, "repeated", [5], [0, -1], lds=1, embed=2)
    assert out["solves"] == 2 and out["embedded"] == 2


@pytest.mark.parametrize("embed", [2, None])
def test_embedded_few_cell_types(tmp_path, embed):
    # full-row relaxations (v and cache_val) beside embedded values; unset: the gate decides (a column in hundreds of caches)
    out = _run(tmp_path, "few_types", [5], [0], lds=1, embed=embed)
    assert out["solves"] == 1 and out["dense_aug"][0] > 0
    assert out["embedded"] == (1 if embed == 2 else out["embedded"]) and out["embedded"] in (0, 1)
