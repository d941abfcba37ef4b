"""Several searches at once (wide_aug<.., PAR>): a search that can no longer be committed -- a lower search of its batch is flagged,
or it is flagged itself -- leaves its rounds early.  That must change nothing but the time: with the developer knob
CYTO_AUG_ABORT on (the default) and off, rowsol, colsol, u, v and the semantic counters equal the wide restatement bit for bit, and
wide_par_batches / wide_par_discarded are the same numbers, the ones tests/test_wide_batch_end_gpu.py holds from the library before
its own change (BATCHES there; copied here where the case exists there).

The knobs are read once per process, so every (case, instantiation, knob) runs in a child interpreter; the restatement's results are
computed once per instance and round cap and shared through a directory of the test session.

The counter of aborted searches (cyto_wide_aborted_searches, process-wide) is 0 with the knob off, at most wide_par_discarded with it
on, and above 0 on the two instances with hundreds of discarded searches: integer ties 400^2 and uniform 2 300^2 at 16 searches
with no round cap.  Why those two must abort: in tests/test_par_abort_cpu.py's model a discarded search above the first flagged one
is aborted at its first poll after the two searches that raise the flag have ended; both instances have batches that discard ten
searches and more, of which only the lowest can be the first flagged one, and the deeper of the others are still in their rounds when
the shallow ones have ended."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (prices, owners in LDS by size | owners only | neither) x (plain | embedded): the five PAR instantiations
CONFIGS = [(2, 0), (1, 0), (1, 2), (0, 0), (0, 2)]

# case -> (searches at once, round caps)
CASES = {
    "ties": ([16], [0, -1]),
    "uniform": ([5, 16], [0, 2, -1]),
    "uniform700": ([16], [0, -1]),
    "repeated": ([5], [0, -1]),
    "few_types": ([5, 16], [0]),
    "tiny": ([2], [0, -1]),
}

# "case/instance/par/rounds" -> [wide_par_batches, wide_par_discarded]: tests/test_wide_batch_end_gpu.py, BATCHES
BATCHES = {
    "uniform/0/5/0": [5, 7], "uniform/0/5/2": [124, 270], "uniform/0/5/-1": [236, 313],
    "uniform/0/16/0": [4, 16], "uniform/0/16/2": [106, 1241], "uniform/0/16/-1": [151, 1439],
    "uniform700/0/16/0": [2, 1], "uniform700/0/16/-1": [61, 614],
    "ties/0/16/0": [60, 591], "ties/0/16/-1": [63, 587],
    "repeated/0/5/0": [87, 234], "repeated/0/5/-1": [312, 1096],
    "few_types/0/5/0": [37, 133],
    "tiny/0/2/0": [0, 0], "tiny/0/2/-1": [1, 0], "tiny/1/2/0": [0, 0], "tiny/1/2/-1": [15, 5], "tiny/2/2/0": [0, 0], "tiny/2/2/-1": [15, 3],
}
MUST_ABORT = {"ties": "ties/0/16/-1", "uniform": "uniform/0/16/-1"}

_WORKER = r'''
import json, os, sys
import numpy as np
from cytospace_amd import _lib
from cytospace_amd.lap import lap_solve

WIDE_KEYS = [("scans_redtransfer", "scans_redtransfer"), ("scans_arr", "scans_arr"), ("scans_aug_init", "scans_aug_init"),
             ("scans_aug_relax", "scans_aug_relax"), ("augmentations", "augmentations"), ("path_hops", "path_hops"),
             ("free_after_colred", "free_after_colred"), ("free_after_arr2", "free_after_arr"), ("wide_rounds", "arr_rounds"),
             ("wide_retired", "arr_retired"), ("wide_scaled", "arr_scaled"), ("wide_phases", "arr_phases")]


def few_types(n):
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


def solve(cache, case, idx, c, r, par):
    o, ostats = reference(cache, case, idx, c, r)
    a0 = _lib.wide_aborted_searches()
    g = lap_solve(c, np.float32, return_info=True, opts=dict(mode=2, wide_rounds=r, wide_par=par))
    for k in ("rowsol", "colsol", "u", "v"):
        assert np.array_equal(g[k], o[k]), (case, c.shape, par, r, k)
    gd = g["info"].as_dict()
    assert gd["wide"] == 1
    for kg, ko in WIDE_KEYS:
        assert gd[kg] == ostats[ko], (case, c.shape, par, r, kg, gd[kg], ostats[ko])
    return [int(gd["wide_par_batches"]), int(gd["wide_par_discarded"]), _lib.wide_aborted_searches() - a0]


def main():
    cache, case, pars, rounds, mode = sys.argv[1], sys.argv[2], json.loads(sys.argv[3]), json.loads(sys.argv[4]), sys.argv[5]
    out = {}
    if mode == "poison":
        # every work buffer arrives filled with the byte: the claim words, P and the labels of a solve are written before they are read
        for byte in (0xFF, 0x7F):
            fills = _lib.cache_poison_fills()
            _lib.cache_poison(byte)
            try:
                for idx, c in enumerate(instances(case)):
                    for r in rounds:
                        for par in pars:
                            out[f"{case}/{idx}/{par}/{r}/{byte}"] = solve(cache, case, idx, c, r, par)
            finally:
                _lib.cache_poison(None)
            assert _lib.cache_poison_fills() > fills
    else:
        for rep in range(2 if mode == "twice" else 1):           # (twice: back to back in one process, the same work buffers again)
            for idx, c in enumerate(instances(case)):
                for r in rounds:
                    for par in pars:
                        res = solve(cache, case, idx, c, r, par)
                        key = f"{case}/{idx}/{par}/{r}"
                        if rep:
                            assert res[:2] == out[key][:2], (key, res, out[key])
                            out[key + "/again"] = res
                        else:
                            out[key] = res
    print(json.dumps({"solves": out, "embedded": _lib.wide_embedded_solves()}))


main()
'''


@pytest.fixture(scope="session")
def reference_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("abort_refs")


def run_case(workdir, cache, case, pars, rounds, lds, embed, abort, mode="plain"):
    script = os.path.join(str(workdir), "abort_worker.py")
    with open(script, "w") as f:
        f.write(_WORKER)
    env = {k: v for k, v in os.environ.items() if k not in ("CYTO_AUG_LDS", "CYTO_AUG_EMBED", "CYTO_AUG_ABORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["CYTO_AUG_LDS"] = str(lds)
    env["CYTO_AUG_EMBED"] = str(embed)
    if abort is not None:                                        # (None: unset, the default -- on)
        env["CYTO_AUG_ABORT"] = str(abort)
    r = subprocess.run([sys.executable, script, str(cache), case, json.dumps(pars), json.dumps(rounds), mode], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, pars, rounds, lds, embed, abort, mode, out)
    return out


def check(case, on, off):
    assert on["solves"].keys() == off["solves"].keys()
    for key, (batches, discarded, aborted) in on["solves"].items():
        b0, d0, a0 = off["solves"][key]
        assert [batches, discarded] == [b0, d0], (key, batches, discarded, b0, d0)
        base = "/".join(key.split("/")[:4])
        if base in BATCHES:
            assert [batches, discarded] == BATCHES[base], (key, batches, discarded, BATCHES[base])
        assert a0 == 0, (key, a0)
        assert 0 <= aborted <= discarded, (key, aborted, discarded)
    if case in MUST_ABORT:
        for key, (batches, discarded, aborted) in on["solves"].items():
            if key.startswith(MUST_ABORT[case]):
                assert discarded > 100 and aborted > 0, (key, discarded, aborted)


@pytest.mark.parametrize("lds,embed", CONFIGS)
@pytest.mark.parametrize("case", list(CASES))
def test_abort_changes_nothing_but_the_time(tmp_path, reference_dir, case, lds, embed):
    pars, rounds = CASES[case]
    on = run_case(tmp_path, reference_dir, case, pars, rounds, lds, embed, 1 if (lds + embed) % 2 else None)
    off = run_case(tmp_path, reference_dir, case, pars, rounds, lds, embed, 0)
    ninst = 3 if case == "tiny" else 1
    assert len(on["solves"]) == ninst * len(pars) * len(rounds)
    for out in (on, off):
        assert out["embedded"] == (len(out["solves"]) if embed == 2 else 0)
    check(case, on, off)


@pytest.mark.parametrize("lds,embed", [(2, 0), (1, 2)])
def test_poisoned_work_buffers(tmp_path, reference_dir, lds, embed):
    on = run_case(tmp_path, reference_dir, "ties", [16], [-1], lds, embed, None, "poison")
    off = run_case(tmp_path, reference_dir, "ties", [16], [-1], lds, embed, 0, "poison")
    assert len(on["solves"]) == 2
    check("ties", on, off)


@pytest.mark.parametrize("lds,embed", [(2, 0), (1, 2)])
def test_two_solves_back_to_back(tmp_path, reference_dir, lds, embed):
    # the claim words and P of a solve that ended with aborted searches do not leak into the next one
    on = run_case(tmp_path, reference_dir, "ties", [16], [-1, 0], lds, embed, None, "twice")
    off = run_case(tmp_path, reference_dir, "ties", [16], [-1, 0], lds, embed, 0, "twice")
    assert len(on["solves"]) == 4
    check("ties", on, off)
    assert on["solves"]["ties/0/16/-1/again"][2] > 0
