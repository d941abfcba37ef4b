"""One conflict flag per wave in the claim pass of the several-searches-at-once kernel (lap_wide.hip: search_end<.., PAR>): a thread
keeps the lowest flagged search it has seen, a wave that saw one sends one atomic min into the batch's P.  Instances in which a later
search of a batch shares MANY columns with an earlier one and is discarded, against the wide restatement and against one search at a
time (wide_par = -1), bit for bit: rowsol, colsol, u, v, the total and the number of searches; and the batches and discarded searches
against the values of the library before this change.

Instances, at n = 65, 700 and 2 300 (a touched list of fewer than 64 entries, of a few hundred, and of more than the 1 024 threads of
the workgroup):
  few_types  six cell types, near-equal columns within a type: deep searches that settle hundreds of the same columns.  The seed is
             chosen on the CPU model below (deep_discard): a batch of `par` searches run from the state after the row reduction
             (oracle.jv.jv_oracle_wide, stop_phase = 2), committed in row order up to the first that meets a lower one's columns; the
             test asserts that the model finds a discarded search sharing more than 64 columns with a lower one of its batch (at
             n = 65 a search cannot settle 64 columns: there the test asks for a discarded search that shares at least nine).
  ties       integer costs 0 ... 9: nearly every batch collides, on a handful of columns each (the model finds no deep discard in
             them: after the row reduction their searches are shallow) -- here for the many P = 1 batches, with the device's own
             count of discarded searches asserted.

CYTO_AUG_LDS and CYTO_AUG_EMBED are read once per process: every knob setting runs in a child interpreter (the pattern of
tests/test_wide_batch_end_gpu.py); the restatement's results are computed once per instance and shared through a directory.

wide_par_batches and wide_par_discarded are a function of the instance and of the number of searches run at once.  Provenance of
BATCHES: a run of the library built from the PARENT of the commit that introduced this file (one atomic min into P per shared
column), on these very instances, under all six knob settings -- which agreed with one another."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

PARS = [2, 5, 16]
SIZES = [65, 700, 2300]
SEED = 1
# CYTO_AUG_LDS x CYTO_AUG_EMBED (None: unset)
CONFIGS = [(lds, emb) for lds in (2, 1) for emb in (0, 2, None)]

# "kind/n/par" -> [wide_par_batches, wide_par_discarded], from the parent commit's library (see the docstring)
BATCHES = {
    "few_types/65/2": [6, 3], "few_types/65/5": [6, 13], "few_types/65/16": [6, 17],
    "few_types/700/2": [24, 13], "few_types/700/5": [23, 71], "few_types/700/16": [23, 227],
    "few_types/2300/2": [50, 41], "few_types/2300/5": [50, 182], "few_types/2300/16": [50, 640],
    "ties/65/2": [11, 5], "ties/65/5": [10, 24], "ties/65/16": [9, 44],
    "ties/700/2": [308, 18], "ties/700/5": [150, 145], "ties/700/16": [114, 1173],
    "ties/2300/2": [1113, 59], "ties/2300/5": [532, 484], "ties/2300/16": [403, 4208],
}


def few_types(n, seed):
    # the generator of tests/test_lap_gpu.py::test_wide_full_row_fallbacks_on_near_equal_columns, with a seed
    rng = np.random.default_rng(seed)
    types = 6
    prof = rng.normal(size=(types, 64)).astype(np.float32)
    rows = prof[rng.integers(0, types, n)] + 0.05 * rng.normal(size=(n, 64)).astype(np.float32)
    cols = prof[rng.integers(0, types, n)] + 0.05 * rng.normal(size=(n, 64)).astype(np.float32)
    return -(rows @ cols.T).astype(np.float32)


def ties(n, seed):
    return np.random.default_rng(seed).integers(0, 10, (n, n)).astype(np.float32)


def instance(kind, n, seed):
    return few_types(n, seed) if kind == "few_types" else ties(n, seed)


# (the child gets the generators as source text: the same instances on both sides)
_WORKER = "import numpy as np\n\n\n" + "\n\n".join(inspect.getsource(f) for f in (few_types, ties, instance)) + r'''
import json, os, sys
from cytospace_amd import _lib
from cytospace_amd.lap import lap_solve


def reference(cache, kind, n, c):
    path = os.path.join(cache, f"{kind}_{n}.npz")
    if os.path.exists(path):
        d = np.load(path)
        return {k: d[k] for k in ("rowsol", "colsol", "u", "v")}, float(d["total"]), int(d["searches"])
    from oracle.jv import jv_oracle_wide
    o = jv_oracle_wide(c, np.float32)
    tmp = path + f".{os.getpid()}.tmp.npz"
    np.savez(tmp, rowsol=o["rowsol"], colsol=o["colsol"], u=o["u"], v=o["v"], total=o["total"], searches=o["stats"].as_dict()["augmentations"])
    os.replace(tmp, path)
    return {k: o[k] for k in ("rowsol", "colsol", "u", "v")}, float(o["total"]), int(o["stats"].as_dict()["augmentations"])


def main():
    cache, seed, sizes, pars = sys.argv[1], int(sys.argv[2]), json.loads(sys.argv[3]), json.loads(sys.argv[4])
    out = {}
    for kind in ("few_types", "ties"):
        for n in sizes:
            c = instance(kind, n, seed)
            o, total, searches = reference(cache, kind, n, c)
            for par in pars + [-1]:
                g = lap_solve(c, np.float32, return_info=True, opts=dict(mode=2, wide_par=par))
                for k in ("rowsol", "colsol", "u", "v"):
                    assert np.array_equal(g[k], o[k]), (kind, n, par, k)
                gd = g["info"].as_dict()
                assert gd["wide"] == 1 and g["total"] == total and gd["augmentations"] == searches, (kind, n, par, g["total"], total)
                out[f"{kind}/{n}/{par}"] = [int(gd["wide_par_batches"]), int(gd["wide_par_discarded"]), searches]
    print(json.dumps(out))


main()
'''


def _search(c, v, colsol, fr):
    """Shortest paths from free row fr over the reduced costs: (columns settled below the end's distance, sink, pred, d, D)."""
    n = c.shape[0]
    d = c[fr].astype(np.float64) - v
    pred = np.full(n, fr)
    done = np.zeros(n, bool)
    while True:
        j = int(np.argmin(np.where(done, np.inf, d)))
        if colsol[j] < 0:
            return np.flatnonzero(done & (d < d[j])), j, pred, d, d[j]
        done[j] = True
        i = colsol[j]
        nd = d[j] + (c[i].astype(np.float64) - v) - (float(c[i, j]) - v[j])
        better = ~done & (nd < d)
        d[better] = nd[better]
        pred[better] = i


def deep_discard(c, G, max_batches=40):
    """The CPU model of the batches: the most columns a discarded search shares with the lower searches of its batch, over the first
    batches of the solve (it stops at the first above 64)."""
    from oracle.jv import jv_oracle_wide
    o = jv_oracle_wide(c, np.float32, max_rounds=-1, stop_phase=2)
    v, rowsol, colsol = o["v"].astype(np.float64), o["rowsol"].copy(), o["colsol"].copy()
    free = [i for i in range(c.shape[0]) if rowsol[i] < 0]
    most = 0
    for _ in range(max_batches):
        if not free:
            break
        res, seen, P = [], set(), None
        for g, fr in enumerate(free[:G]):
            settled, sink, pred, d, D = _search(c, v, colsol, fr)
            mine = set(settled.tolist()) | {sink}
            shared = len(mine & seen)
            if shared and P is None:
                P = g
            if P is not None:
                most = max(most, shared)
                if most > 64:
                    return most
            seen |= mine
            res.append((fr, settled, sink, pred, d, D))
        for fr, settled, sink, pred, d, D in res[:len(res) if P is None else P]:
            v[settled] += d[settled] - D
            j = sink
            while True:
                i = pred[j]
                colsol[j] = i
                j, rowsol[i] = rowsol[i], j
                if i == fr:
                    break
        free = free[len(res) if P is None else P:]
    return most


@pytest.fixture(scope="session")
def reference_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("claim_flag_refs")


@pytest.mark.parametrize("par", PARS)
def test_the_instances_discard_deep_searches(par):
    # (no GPU work: the choice of SEED, held against the model)
    assert deep_discard(instance("few_types", 65, SEED), par) >= 9
    assert deep_discard(instance("few_types", 700, SEED), par) > 64
    assert deep_discard(instance("few_types", 2300, SEED), par) > 64


@pytest.mark.parametrize("lds,embed", CONFIGS)
def test_claim_flags(tmp_path, reference_dir, lds, embed):
    script = tmp_path / "claim_flags_worker.py"
    script.write_text(_WORKER)
    env = {k: v for k, v in os.environ.items() if k not in ("CYTO_AUG_LDS", "CYTO_AUG_EMBED")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["CYTO_AUG_LDS"] = str(lds)
    if embed is not None:
        env["CYTO_AUG_EMBED"] = str(embed)
    r = subprocess.run([sys.executable, str(script), str(reference_dir), str(SEED), json.dumps(SIZES), json.dumps(PARS)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(lds, embed, json.dumps(out))
    assert len(out) == 2 * len(SIZES) * (len(PARS) + 1)
    for key, (batches, discarded, searches) in out.items():
        kind, n, par = key.split("/")
        if int(par) < 0:
            assert batches == 0 and discarded == 0 and searches > 0, key
            continue
        assert [batches, discarded] == BATCHES[key], (key, batches, discarded, BATCHES[key])
        assert batches <= searches <= batches * int(par) and discarded <= batches * (int(par) - 1), key
        if int(n) >= 700:
            assert discarded > 0, key
