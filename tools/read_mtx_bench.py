"""read_mtx_device (the device MatrixMarket reader, csrc/mtx_read.hip) against read_file(keep_sparse=False) (scipy's mmread, then
pandas' sparse frame made dense) on a 10x directory.

  python tools/read_mtx_bench.py [--genes 5000] [--cells 20000] [--reps 5] [--no-host] [--out DIR]

Input: genes x cells Poisson(0.4) counts -- the matrix of tools/read_table_bench.py -- as an `integer` MatrixMarket file with
genes.tsv and barcodes.tsv beside it, in a temporary directory (written by the device writer, post_processing.write_mtx_device:
scipy's bytes).  Timed with a host clock around the whole call, the file in the page cache (read once before), after a small
warm-up call: `reps` device calls and two read_file calls (min / median / max), the results compared with assert_frame_equal
(exact), and the device's phase split (the median over the calls of every phase read_mtx_device reports).
One JSON line; with --out it is appended to DIR/read_mtx_bench.jsonl."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("labels_s", "header_s", "file_read_s", "upload_s", "kernels_s", "download_s", "dataframe_s", "total_s")


def write_input(d, G, C, seed=0):
    """The 10x directory d; returns (path of matrix.mtx, its size, its entries)."""
    from cytospace_amd.post_processing import write_mtx_device
    os.makedirs(d, exist_ok=True)
    x = np.random.default_rng(seed).poisson(0.4, (G, C)).astype(np.int64)
    p = os.path.join(d, "matrix.mtx")
    info = write_mtx_device(p, x, np.arange(C), return_info=True)
    assert info["path"] == "device", info
    with open(os.path.join(d, "genes.tsv"), "w") as f:
        f.write("".join(f"gene{g}\n" for g in range(G)))
    with open(os.path.join(d, "barcodes.tsv"), "w") as f:
        f.write("".join(f"cell{j}\n" for j in range(C)))
    return p, os.path.getsize(p), int(np.count_nonzero(x))


def page_in(path):
    with open(path, "rb") as f:
        while f.read(64 << 20):
            pass


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def spread(ts):
    return {"min": round(min(ts), 3), "median": round(float(np.median(ts)), 3), "max": round(max(ts), 3), "n": len(ts)}


def device_calls(path, reps):
    from cytospace_amd.common import read_mtx_device
    ts, infos, df = [], [], None
    for _ in range(reps):
        df = None
        (df, info), t = timed(lambda: read_mtx_device(path, return_info=True))
        assert info["path"] == "device", info
        ts.append(t)
        infos.append(info)
    ph = {k: round(float(np.median([i[k] for i in infos])), 4) for k in PHASES}
    ph["outside_phases_s"] = round(float(np.median([i["total_s"] - sum(i[k] for k in PHASES[:-1]) for i in infos])), 4)
    return df, ts, ph


def bench(G, C, host, d, reps):
    import ctypes
    import pandas as pd
    from cytospace_amd import _lib
    from cytospace_amd.common import read_file, read_mtx_device
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().cyto_device_name(0, name, 256))
    out = {"device": name.value.decode()}
    warm, _, _ = write_input(os.path.join(d, "warm"), 50, 300)
    read_mtx_device(warm)                                                # warm-up: library, HIP, kernels

    p, size, nnz = write_input(os.path.join(d, "bench"), G, C)
    leg = {"genes": G, "cells": C, "entries": nnz, "bytes": size}
    page_in(p)
    dev, ts, ph = device_calls(p, reps)
    leg.update(device_s=spread(ts), phases=ph)
    if host:
        hs = []
        for _ in range(2):
            want = None
            want, t_host = timed(lambda: read_file(p, keep_sparse=False))
            hs.append(t_host)
        pd.testing.assert_frame_equal(dev, want, check_exact=True)
        leg.update(host_s=spread(hs), speedup_median=round(float(np.median(hs) / np.median(ts)), 1), equal=True)
    out["mtx"] = leg
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=5000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="read_mtx_bench_")
    try:
        res = bench(a.genes, a.cells, not a.no_host, d, a.reps)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "read_mtx_bench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
