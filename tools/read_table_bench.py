"""read_file_device (the device table reader, csrc/table.hip) against read_file (pandas) on dense tab-separated count tables.

  python tools/read_table_bench.py [--genes 5000] [--cells 20000] [--reps 5] [--big-genes 20000 --big-cells 50000] [--no-host]
                                   [--out DIR]

Input: genes x cells Poisson(0.4) counts (capped at 9), gene names in the first column and cell ids in the header, as R's
write.table(..., sep='\\t', quote=F) writes them (one header field fewer than the data lines), in a temporary directory.
Timed with a host clock around the whole call, the file in the page cache (read once before), after a small warm-up call.
Legs: `genes` x `cells` on both paths (`reps` device calls and two host calls: min / median / max; results compared with
assert_frame_equal, exact), the device alone at `big_genes` x `big_cells` (skipped when either is 0), and the device's phase split
(the median over the calls of every phase read_file_device reports).
One JSON line; with --out it is appended to DIR/read_table_bench.jsonl."""
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


def write_table(path, G, C, seed=0):
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        f.write(("\t".join(f"cell{j}" for j in range(C)) + "\n").encode())
        row = np.empty(2 * C + 1, np.uint8)
        row[0:2 * C:2] = ord("\t")
        row[2 * C] = ord("\n")
        for g in range(G):
            row[1:2 * C:2] = ord("0") + np.minimum(rng.poisson(0.4, C), 9)
            f.write(f"gene{g}".encode())
            f.write(row.tobytes())
    return os.path.getsize(path)


def page_in(path):
    with open(path, "rb") as f:
        while f.read(64 << 20):
            pass


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


PHASES = ("header_s", "file_read_s", "upload_s", "kernels_s", "device_setup_s", "download_s", "free_s", "dataframe_s", "total_s")


def spread(ts):
    return {"min": round(min(ts), 3), "median": round(float(np.median(ts)), 3), "max": round(max(ts), 3), "n": len(ts)}


def device_calls(path, reps):
    from cytospace_amd.common import read_file_device
    ts, infos, df = [], [], None
    for _ in range(reps):
        df = None
        (df, info), t = timed(lambda: read_file_device(path, return_info=True))
        assert info["path"] == "device", info
        ts.append(t)
        infos.append(info)
    ph = {k: round(float(np.median([i[k] for i in infos])), 4) for k in PHASES}
    ph["outside_phases_s"] = round(float(np.median([i["total_s"] - sum(i[k] for k in PHASES[:-1]) for i in infos])), 4)
    return df, ts, ph


def bench(G, C, big_G, big_C, host, d, reps):
    import ctypes
    import pandas as pd
    from cytospace_amd import _lib
    from cytospace_amd.common import read_file, read_file_device
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().cyto_device_name(0, name, 256))
    out = {"device": name.value.decode()}
    warm = os.path.join(d, "warm.tsv")
    write_table(warm, 50, 300)
    read_file_device(warm)                                               # warm-up: library, HIP, kernels

    p = os.path.join(d, "table.tsv")
    leg = {"genes": G, "cells": C, "bytes": write_table(p, G, C)}
    page_in(p)
    dev, ts, ph = device_calls(p, reps)
    leg.update(device_s=spread(ts), phases=ph)
    if host:
        hs = []
        for _ in range(2):
            want, t_host = timed(lambda: read_file(p))
            hs.append(t_host)
        pd.testing.assert_frame_equal(dev, want, check_exact=True)
        leg.update(host_s=spread(hs), speedup_median=round(float(np.median(hs) / np.median(ts)), 1), equal=True)
    out["table"] = leg
    del dev
    os.remove(p)

    if big_G and big_C:
        q = os.path.join(d, "big.tsv")
        big = {"genes": big_G, "cells": big_C, "bytes": write_table(q, big_G, big_C, seed=1)}
        page_in(q)
        db, tb, pb = device_calls(q, 2)
        big.update(device_s=spread(tb), phases=pb, shape=list(db.shape))
        out["big"] = big
        del db
        os.remove(q)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=5000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--big-genes", type=int, default=0)
    ap.add_argument("--big-cells", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="read_table_bench_")
    try:
        res = bench(a.genes, a.cells, a.big_genes, a.big_cells, not a.no_host, d, a.reps)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "read_table_bench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
