"""The end of a batch of the several-searches-at-once kernel (wide_aug<.., PAR>: claims that flag a conflict when they arrive, one
list of settled columns per search, the path walked beside the price update) and of the one-search-at-a-time kernel that shares
the update, walk and reset, against the wide restatement, bit for bit: rowsol, colsol, u, v and the semantic counters.

The knobs that select the instantiation (CYTO_AUG_LDS, CYTO_AUG_EMBED) are read once per process, so every case runs in a child
interpreter (the pattern of tests/test_wide_embedded_gpu.py).  The restatement's results are computed once per instance and round cap
and shared by the children through a directory of the test session.

wide_par_batches and wide_par_discarded are deterministic (a function of the instance, the round cap and the number of searches
run at once -- not of where the arrays live): they are held against BATCHES below.  Provenance of these constants: a run of the
library built from the PARENT of the commit that introduced this file (its batch end: non-returning claims, a check pass behind a
grid barrier), on these very instances, under all five knob settings -- which agreed with one another."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (prices, owners in LDS by size | owners only | neither) x (plain | embedded, which needs the prices out of LDS): the five PAR instantiations
CONFIGS = [(2, 0), (1, 0), (1, 2), (0, 0), (0, 2)]

# case -> (searches at once, round caps)
CASES = {
    "uniform": ([2, 5, 16], [0, 2, -1]),       # wide_rounds = -1: about n / e searches, hundreds of batches
    "uniform700": ([2, 16], [0, -1]),
    "ties": ([16], [0, -1]),                   # integer costs 0 ... 9: nearly every batch collides; P = 1 batches; discarded searches log nothing
    "repeated": ([5], [0, -1]),                # 150 distinct rows x 4
    "few_types": ([5], [0]),                   # full-row relaxations beside the list of settled columns
    "tiny": ([2], [0, -1]),                    # n = 3, 64, 65
}

# "case/instance/par/rounds" -> [wide_par_batches, wide_par_discarded], from the parent commit's library (see the docstring)
BATCHES = {
    "uniform/0/2/0": [9, 1], "uniform/0/2/2": [194, 47], "uniform/0/2/-1": [463, 68],
    "uniform/0/5/0": [5, 7], "uniform/0/5/2": [124, 270], "uniform/0/5/-1": [236, 313],
    "uniform/0/16/0": [4, 16], "uniform/0/16/2": [106, 1241], "uniform/0/16/-1": [151, 1439],
    "uniform700/0/2/0": [2, 0], "uniform700/0/2/-1": [138, 30], "uniform700/0/16/0": [2, 1], "uniform700/0/16/-1": [61, 614],
    "ties/0/16/0": [60, 591], "ties/0/16/-1": [63, 587],
    "repeated/0/5/0": [87, 234], "repeated/0/5/-1": [312, 1096],
    "few_types/0/5/0": [37, 133],
    "tiny/0/2/0": [0, 0], "tiny/0/2/-1": [1, 0], "tiny/1/2/0": [0, 0], "tiny/1/2/-1": [15, 5], "tiny/2/2/0": [0, 0], "tiny/2/2/-1": [15, 3],
}

_WORKER = r'''
import json, os, sys
import numpy as np
from cytospace_amd import _lib
from cytospace_amd.lap import lap_solve

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


def reference(cache, case, idx, c, r):
    """The restatement's result for instance idx of the case at round cap r: computed by the first child that needs it."""
    path = os.path.join(cache, f"{case}_{idx}_{r}.npz")
    if os.path.exists(path):
        d = np.load(path)
        return {k: d[k] for k in ("rowsol", "colsol", "u", "v")}, json.loads(str(d["stats"]))
    from oracle.jv import jv_oracle_wide
    o = jv_oracle_wide(c, np.float32, max_rounds=-1 if r == 0 else max(r, 0))
    od = o["stats"].as_dict()
    stats = {ko: int(od[ko]) for _, ko in WIDE_KEYS}
    tmp = path + f".{os.getpid()}.tmp.npz"
    np.savez(tmp, rowsol=o["rowsol"], colsol=o["colsol"], u=o["u"], v=o["v"], stats=json.dumps(stats))
    os.replace(tmp, path)
    return {k: o[k] for k in ("rowsol", "colsol", "u", "v")}, stats


def main():
    cache, case, pars, rounds = sys.argv[1], sys.argv[2], json.loads(sys.argv[3]), json.loads(sys.argv[4])
    before = _lib.wide_embedded_solves()
    out = {}
    for idx, c in enumerate(instances(case)):
        for r in rounds:
            o, ostats = reference(cache, case, idx, c, r)
            for par in pars:
                g = lap_solve(c, np.float32, return_info=True, opts=dict(mode=2, wide_rounds=r, wide_par=par))
                for k in ("rowsol", "colsol", "u", "v"):
                    assert np.array_equal(g[k], o[k]), (case, c.shape, par, r, k)
                gd = g["info"].as_dict()
                assert gd["wide"] == 1
                for kg, ko in WIDE_KEYS:
                    assert gd[kg] == ostats[ko], (case, c.shape, par, r, kg, gd[kg], ostats[ko])
                out[f"{case}/{idx}/{par}/{r}"] = [int(gd["wide_par_batches"]), int(gd["wide_par_discarded"]), int(gd["augmentations"]),
                                                 int(gd["wide_dense_aug"])]
    print(json.dumps({"solves": out, "embedded": _lib.wide_embedded_solves() - before}))


main()
'''


@pytest.fixture(scope="session")
def reference_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("batch_end_refs")


def run_case(workdir, cache, case, pars, rounds, lds, embed):
    script = os.path.join(str(workdir), "batch_end_worker.py")
    with open(script, "w") as f:
        f.write(_WORKER)
    env = {k: v for k, v in os.environ.items() if k not in ("CYTO_AUG_LDS", "CYTO_AUG_EMBED")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["CYTO_AUG_LDS"] = str(lds)
    env["CYTO_AUG_EMBED"] = str(embed)
    r = subprocess.run([sys.executable, script, str(cache), case, json.dumps(pars), json.dumps(rounds)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, pars, rounds, lds, embed, out)
    return out


@pytest.mark.parametrize("lds,embed", CONFIGS)
@pytest.mark.parametrize("case", list(CASES))
def test_batch_end(tmp_path, reference_dir, case, lds, embed):
    pars, rounds = CASES[case]
    out = run_case(tmp_path, reference_dir, case, pars, rounds, lds, embed)
    ninst = 3 if case == "tiny" else 1
    assert len(out["solves"]) == ninst * len(pars) * len(rounds)
    assert out["embedded"] == (len(out["solves"]) if embed == 2 else 0)
    for key, (batches, discarded, searches, dense_aug) in out["solves"].items():
        assert [batches, discarded] == BATCHES[key], (key, batches, discarded, BATCHES[key])
        par = int(key.split("/")[2])
        # every batch commits at least its first search and at most `par`; what it does not commit is discarded, the last batch's idle
        # workgroups aside
        assert batches <= searches <= batches * par and discarded <= batches * (par - 1), (key, batches, discarded, searches)
    if case == "uniform":
        assert out["solves"]["uniform/0/16/-1"][2] > 2300 // 5      # (the column reduction of a uniform instance leaves about n / e rows free)
        assert out["solves"]["uniform/0/2/-1"][0] > 200             # hundreds of batches
    if case == "ties":
        assert out["solves"]["ties/0/16/-1"][1] > 0                 # searches were discarded
    if case == "few_types":
        assert out["solves"]["few_types/0/5/0"][3] > 0              # full-row relaxations


@pytest.mark.parametrize("case,par", [("few_types", 0), ("uniform700", 0), ("uniform", -1)])
def test_one_search_at_a_time(tmp_path, reference_dir, case, par):
    # the kernel of the batched legs (PAR = false) shares the update, the walk and the reset: wide_par = 0 below 2 048 rows, -1 anywhere
    out = run_case(tmp_path, reference_dir, case, [par], [0, -1] if case != "few_types" else [0], 2, 0)
    for key, (batches, discarded, searches, dense_aug) in out["solves"].items():
        assert batches == 0 and discarded == 0 and searches > 0, (key, batches, discarded, searches)
