"""The gate of the embedded form, taken on the device (lap_wide_drv.hip: wide_solve_batch enqueues wide_aug<.., EMB> and its plain twin
back to back behind the build of the inverse lists; each reads the longest list and the one whose turn it is not returns at once;
which one ran comes back in the status block and moves cyto_wide_embedded_solves()).

CYTO_AUG_EMBED is read once per process, so every case runs in a child interpreter (the pattern of tests/test_wide_embedded_gpu.py).

What the gate reads is the longest inverse list: in how many rows' caches a column lies.  A cache holds the columns of a row with
c - v below a floor, the lowest ones first: at most 63 of them, and by the builders' contract at least 16 (fewer: the row is built
again or falls back to its full row).  So, for the prices the caches of the searches are built against -- the column minima (the
first build) or the prices behind the row reduction (a rebuild; oracle.jv.jv_oracle_wide, stop_phase = 2; the row reduction is
capped at two rounds in every case here, so that dozens of searches are left at every size) --
    lower(c) = min over both price vectors of  max_j #{ rows i : j is among the 16 lowest c[i] - v }  <=  longest
    upper(c) = max over both price vectors of  max_j #{ rows i : j is among the 63 lowest c[i] - v }  >=  longest
(ties at the 16th / 63rd place aside: the instances are continuous).  The uniform instance has upper <= EMB_GATE / 2: the gate is
open.  For the instance that must take the PLAIN kernel the child takes the smallest n of a ladder with lower > EMB_GATE.
The few-cell-type generators of the other wide tests cannot serve for it at a test's size: at n = 400 ... 2 300 their upper bound
behind the row reduction is 104 ... 281 and their lower bound 40 ... 74 (six, two and one type measured), so nothing proves a list
above 252 -- and the device does take the embedded kernel on them.  What the gate is there for, "one column in thousands of
caches", is built directly instead: a uniform cost in which ONE column costs the same in every row, so that its reduced cost is the
same in every row whatever its price, and below nearly every other column's in nearly every row (lower = 260 at n = 260)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMB_GATE = 4 * 63

_WORKER = r'''
import json, sys
import numpy as np
from cytospace_amd import _lib
from cytospace_amd.lap import lap_solve
from oracle.jv import jv_oracle_wide

EMB_GATE = 4 * 63
ROUNDS = 2          # cap on the row-reduction rounds (cyto_lap_opts.wide_rounds): dozens of searches are left at every size


def in_lowest(c, v, k):
    k = min(k, c.shape[0] - 1)
    idx = np.argpartition(c - v[None, :], k - 1, axis=1)[:, :k]
    return int(np.bincount(idx.ravel(), minlength=c.shape[0]).max())


def bounds(c):
    """(lower, upper) bounds of the longest inverse list, see the test module's docstring."""
    vs = (c.min(axis=0), jv_oracle_wide(c, np.float32, max_rounds=ROUNDS, stop_phase=2)["v"])
    return min(in_lowest(c, v, 16) for v in vs), max(in_lowest(c, v, 63) for v in vs)


def one_flat_column(n):
    c = np.random.default_rng(42).random((n, n)).astype(np.float32)
    c[:, 0] = -1.0
    return c


def crowded():
    for n in (200, 260, 300, 400, 600):
        c = one_flat_column(n)
        lo, up = bounds(c)
        if lo > EMB_GATE:
            return c, (lo, up)
    raise SystemExit("no instance of the ladder has a column in provably more than EMB_GATE caches")


def main():
    case = sys.argv[1]
    if case == "uniform":
        c = np.random.default_rng(42).random((2300, 2300)).astype(np.float32)
        counts = bounds(c)
    else:
        c, counts = crowded()
    o = jv_oracle_wide(c, np.float32, max_rounds=ROUNDS)
    assert o["stats"].as_dict()["augmentations"] >= 16          # searches for more than one batch
    moved = []
    for rep in range(2):                     # the second solve needs the slot of the several-searches-at-once kernel again
        before = _lib.wide_embedded_solves()
        g = lap_solve(c, np.float32, return_info=True, opts=dict(mode=2, wide_rounds=ROUNDS, wide_par=16))
        for k in ("rowsol", "colsol", "u", "v"):
            assert np.array_equal(g[k], o[k]), (case, c.shape, rep, k)
        assert g["total"] == o["total"]
        gd = g["info"].as_dict()
        assert gd["wide"] == 1 and gd["augmentations"] == o["stats"].as_dict()["augmentations"]
        assert gd["wide_par_batches"] > 0, "the second solve did not get the slot: one search at a time"
        moved.append(_lib.wide_embedded_solves() - before)
    print(json.dumps({"n": int(c.shape[0]), "counts": counts, "moved": moved}))


main()
'''


def _run(tmp_path, case, embed):
    script = tmp_path / "embed_gate_worker.py"
    script.write_text(_WORKER)
    env = {k: v for k, v in os.environ.items() if k not in ("CYTO_AUG_LDS", "CYTO_AUG_EMBED")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["CYTO_AUG_LDS"] = "1"                # prices in global memory: where the embedded form can run at these sizes
    if embed is not None:
        env["CYTO_AUG_EMBED"] = str(embed)
    r = subprocess.run([sys.executable, str(script), case], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, embed, out)
    return out


@pytest.mark.parametrize("embed", [None, 1])
def test_gate_open_takes_the_embedded_kernel(tmp_path, embed):
    out = _run(tmp_path, "uniform", embed)
    assert out["n"] == 2300 and out["counts"][1] <= EMB_GATE // 2      # (about 63 caches per column, no list of twice that)
    assert out["moved"] == [1, 1]


@pytest.mark.parametrize("embed", [None, 1])
def test_gate_shut_takes_the_plain_kernel(tmp_path, embed):
    out = _run(tmp_path, "crowded", embed)
    assert out["counts"][0] > EMB_GATE
    assert out["moved"] == [0, 0]


@pytest.mark.parametrize("case", ["uniform", "crowded"])
def test_knobs_zero_and_two_do_not_ask_the_device(tmp_path, case):
    assert _run(tmp_path, case, 0)["moved"] == [0, 0]
    assert _run(tmp_path, case, 2)["moved"] == [1, 1]
