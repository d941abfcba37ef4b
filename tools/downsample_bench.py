"""downsample_device against the host `downsample` (cytospace_amd/common.py) at production sizes, and one command-line run.

  python tools/downsample_bench.py [--cells 50000] [--big-cells 200000] [--out DIR]      GPU: one JSON line
  python tools/downsample_bench.py --cli-run DIR                                         GPU: python -m cytospace_amd on a
                                                                                         synthetic 5 000 genes x 20 000 cells set

Input: 20 000 genes x N cells, lognormal gene rates, about 6 000 UMIs per cell (1 000 distinct cells tiled), target 1 500.
Timed with a host clock around the whole call (upload, kernels, download, the DataFrame), after a small warm-up call.
Legs: `cells` with int64 counts on both paths (host and device; results compared), the device alone with uint16 counts in and
out at `cells`, and the device alone at `big_cells` with uint16 counts (the host's int64 result there would be 32 GB: its time
is extrapolated from the per-cell time of the first leg)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def counts(G, C, umis=6000, distinct=1000, seed=0, dtype=np.int64):
    rng = np.random.default_rng(seed)
    rate = rng.lognormal(0, 1.5, G)
    rate *= umis / rate.sum()
    base = rng.poisson(rate[:, None] * rng.lognormal(0, 0.3, (1, distinct))).astype(dtype)
    return np.tile(base, (1, -(-C // distinct)))[:, :C]


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def bench(cells, big_cells, target=1500, G=20000):
    from cytospace_amd import _lib
    from cytospace_amd.common import downsample, downsample_device
    import ctypes
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().cyto_device_name(0, name, 256))
    out = {"device": name.value.decode(), "genes": G, "target": target}
    np.random.seed(0)
    downsample_device(pd.DataFrame(counts(200, 50, umis=3000)), target)                 # warm-up: library, HIP, kernels

    x = pd.DataFrame(counts(G, cells))
    out["cells"] = cells
    out["mean_umis_per_cell"] = round(float(x.iloc[:, :1000].sum().mean()), 1)
    np.random.seed(1)
    (dev, words), t_dev = timed(lambda: downsample_device(x, target, return_words=True))
    s_dev = np.random.get_state()
    np.random.seed(1)
    host, t_host = timed(lambda: downsample(x, target))
    s_host = np.random.get_state()
    out["int64"] = {"device_s": round(t_dev, 3), "host_s": round(t_host, 3), "speedup": round(t_host / t_dev, 1), "words": int(words),
                    "equal": bool(np.array_equal(dev.to_numpy(), host.to_numpy()) and np.array_equal(s_dev[1], s_host[1])
                                  and s_dev[2] == s_host[2])}
    host_per_cell = t_host / cells
    del dev, host, x

    x16 = pd.DataFrame(counts(G, cells, dtype=np.uint16))
    np.random.seed(1)
    (d16, w16), t16 = timed(lambda: downsample_device(x16, target, dtype=np.uint16, return_words=True))
    out["uint16"] = {"device_s": round(t16, 3), "words": int(w16), "speedup_vs_host_int64": round(t_host / t16, 1)}
    del d16, x16

    if big_cells:
        xb = pd.DataFrame(counts(G, big_cells, dtype=np.uint16))
        np.random.seed(1)
        (db, wb), tb = timed(lambda: downsample_device(xb, target, dtype=np.uint16, return_words=True))
        out["big"] = {"cells": big_cells, "device_s": round(tb, 3), "words": int(wb),
                      "host_s_extrapolated": round(host_per_cell * big_cells, 1),
                      "speedup_vs_extrapolated_host": round(host_per_cell * big_cells / tb, 1)}
    return out


def cli_run(d, G=5000, C=20000, S=2000, seed=3):
    """Synthetic inputs (scRNA as MatrixMarket, the rest as csv) and one `python -m cytospace_amd` run; returns its wall time."""
    import scipy.io
    import scipy.sparse as sp
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    K = 6
    rate = rng.lognormal(0, 1.5, G)
    prof = rng.lognormal(0, 1.0, (K, G)) * rate
    prof /= prof.sum(1, keepdims=True)
    ctype = rng.integers(0, K, C)
    sc = rng.poisson(prof[ctype].T * rng.lognormal(np.log(4000), 0.4, C))
    genes = [f"g{i}" for i in range(G)]
    scipy.io.mmwrite(os.path.join(d, "matrix.mtx"), sp.csc_matrix(sc))
    pd.Series(genes).to_csv(os.path.join(d, "genes.tsv"), sep="\t", header=False, index=False)
    pd.Series([f"c{i}" for i in range(C)]).to_csv(os.path.join(d, "barcodes.tsv"), sep="\t", header=False, index=False)
    names = [f"type{k}" for k in range(K)]
    pd.DataFrame({"CellType": [names[t] for t in ctype]}, index=pd.Index([f"c{i}" for i in range(C)], name="ID")).to_csv(
        os.path.join(d, "cell_types.csv"))
    mix = rng.dirichlet(np.ones(K), S)
    st = rng.poisson((mix @ prof).T * 5 * 4000)
    spots = [f"s{i}" for i in range(S)]
    pd.DataFrame(st, index=pd.Index(genes, name="ID"), columns=spots).to_csv(os.path.join(d, "st.csv"))
    pd.DataFrame({"row": np.arange(S) // 50, "col": np.arange(S) % 50}, index=pd.Index(spots, name="ID")).to_csv(os.path.join(d, "coords.csv"))
    pd.DataFrame([mix.mean(0)], index=["Fraction"], columns=names).to_csv(os.path.join(d, "fractions.csv"))
    argv = [sys.executable, "-m", "cytospace_amd", "-sp", "./matrix.mtx", "-ctp", "cell_types.csv", "-stp", "st.csv", "-cp", "coords.csv",
            "-ctfep", "fractions.csv", "-o", "out", "-p"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t = time.perf_counter()
    r = subprocess.run(argv, cwd=d, env=env, capture_output=True, text=True, timeout=1800)
    wall = time.perf_counter() - t
    sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit(f"cli run failed with {r.returncode}")
    return {"cli_wall_s": round(wall, 2), "genes": G, "cells": C, "spots": S, "log": os.path.join(d, "out", "log.txt")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--big-cells", type=int, default=200000)
    ap.add_argument("--cli-run", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = cli_run(a.cli_run) if a.cli_run else bench(a.cells, a.big_cells)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "downsample_bench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
