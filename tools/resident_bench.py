"""main_cytospace with the expression tables resident on the GPU (resident=True: cytospace_amd/resident.py)
against the same call with the switch off, on one synthetic input set.

  python tools/resident_bench.py [--genes 5000] [--cells 20000] [--spots 2000] [--types 8] [--reps 5] [--seed 0] [--out DIR]

Input, from the seed: genes x cells Poisson counts of mean 0.4 (the matrix size of tools/read_mtx_bench.py; every cell type has
its own gene profile), spots that are Poisson sums of five profiles, a cell-type table, a fractions file and coordinates, all as
.csv in a temporary directory (the two expression tables written by post_processing.write_csv_device).  The cells per spot are
estimated (mean 5), sampling is `duplicates`, one LAP.

The two legs run alternately in one process -- host, resident, host, resident, ... --, one warm-up each, then `reps` each, timed
with the host clock around the whole call (every run ends in its file writes, after the device work).  The host leg is the code
path the package had before the switch existed, so the alternation is the comparison.  After the last pair the two output folders
are compared byte for byte (log.txt aside).  One JSON line: min / median / max per leg, the per-frame reports of
resident.last_run and the device name; with --out it is appended to DIR/resident_bench.jsonl."""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_inputs(d, G, C, S, T, seed):
    """The input files in d; returns main_cytospace's path arguments."""
    import pandas as pd
    from cytospace_amd.post_processing import write_csv_device
    rng = np.random.default_rng(seed)
    profiles = rng.gamma(0.5, 0.8, (G, T))                   # mean 0.4 per gene and type
    types = rng.integers(0, T, C)
    sc = rng.poisson(profiles[:, types]).astype(np.int64)
    mix = np.zeros((T, S))
    for k in range(5):
        mix[rng.integers(0, T, S), np.arange(S)] += 1.0
    st = rng.poisson(profiles @ mix).astype(np.int64)
    genes = [f"gene{g}" for g in range(G)]
    cells, spots = [f"cell{j}" for j in range(C)], [f"spot{j}" for j in range(S)]
    paths = {k: os.path.join(d, k + ".csv") for k in ("scRNA", "st", "cell_types", "fractions", "coords")}
    for name, x, cols in (("scRNA", sc, cells), ("st", st, spots)):
        info = write_csv_device(paths[name], x, np.arange(x.shape[1]), index_labels=genes, column_labels=cols, index_name="GENES",
                                return_info=True)
        assert info["path"] == "device", info
    pd.DataFrame({"CellType": [f"type{t}" for t in types]}, index=pd.Index(cells, name="Cell IDs")).to_csv(paths["cell_types"])
    frac = np.bincount(types, minlength=T) / C
    pd.DataFrame([frac], index=pd.Index(["Fraction"], name="Index"), columns=[f"type{t}" for t in range(T)]).to_csv(paths["fractions"])
    pd.DataFrame({"row": np.arange(S) // 50, "col": np.arange(S) % 50}, index=pd.Index(spots, name="SpotID")).to_csv(paths["coords"])
    return dict(scRNA_path=paths["scRNA"], cell_type_path=paths["cell_types"], n_cells_per_spot_path=None, st_cell_type_path=None,
                cell_type_fraction_estimation_path=paths["fractions"], st_path=paths["st"], coordinates_path=paths["coords"])


def folder(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            if f != "log.txt":
                out[os.path.relpath(os.path.join(root, f), d)] = open(os.path.join(root, f), "rb").read()
    return out


def spread(ts):
    return {"min": round(min(ts), 3), "median": round(float(np.median(ts)), 3), "max": round(max(ts), 3), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=5000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--spots", type=int, default=2000)
    ap.add_argument("--types", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    from cytospace_amd import _lib, resident
    from cytospace_amd.cytospace import main_cytospace
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().cyto_device_name(0, name, 256))
    d = tempfile.mkdtemp(prefix="resident_bench_")
    try:
        args = write_inputs(d, a.genes, a.cells, a.spots, a.types, a.seed)
        sizes = {k: os.path.getsize(args[k]) for k in ("scRNA_path", "st_path")}
        times = {"host": [], "resident": []}
        report = None
        for rep in range(a.reps + 1):                        # rep 0: the warm-up pair
            for leg in ("host", "resident"):
                out = os.path.join(d, "out_" + leg)
                shutil.rmtree(out, ignore_errors=True)
                t = time.perf_counter()
                main_cytospace(**args, output_folder=out, seed=1, plot_off=True, devices=[0], resident=(leg == "resident"))
                dt = time.perf_counter() - t
                if rep:
                    times[leg].append(dt)
                if leg == "resident":
                    report = json.loads(json.dumps(resident.last_run))
        a_files, b_files = folder(os.path.join(d, "out_host")), folder(os.path.join(d, "out_resident"))
        equal = sorted(a_files) == sorted(b_files) and all(a_files[k] == b_files[k] for k in a_files)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    h, r = spread(times["host"]), spread(times["resident"])
    rec = {"device": name.value.decode(), "genes": a.genes, "cells": a.cells, "spots": a.spots, "types": a.types, "seed": a.seed,
           "input_bytes": sizes, "host_s": h, "resident_s": r, "median_ratio_host_over_resident": round(h["median"] / r["median"], 3),
           "outputs_equal": bool(equal), "last_run": report}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "resident_bench.jsonl"), "a") as f:
            f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
