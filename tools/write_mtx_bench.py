"""write_mtx_device (the device MatrixMarket writer, csrc/mtx.hip) against the host path of save_results (DataFrame.loc,
scipy.sparse.coo_matrix, scipy.io.mmwrite) on the same frame in the same process.

  python tools/write_mtx_bench.py [--genes 5000] [--cells 8000] [--assigned 20000] [--density 0.1] [--reps 5] [--host-reps 5]
                                  [--big-genes 20000 --big-cells 50000 --big-assigned 50000] [--block-bytes 0] [--out DIR]
                                  [--fractions [--dtype float64|float32]] [--pass-flag]

Input: genes x cells Poisson counts whose share of non-zeros is `density` (int64, as the table reader gives them), labelled
GENE_* / CELL_*; `assigned` cells drawn with replacement.  Timed with a host clock around the whole call (the device call ends after
its last write()), into a temporary directory, after a small warm-up call of each path; the two paths' calls alternate.  Legs: both
paths at genes x cells (min / median / max, the files compared byte for byte, the device's phase split as the median over its calls,
the format pass's share in bytes of text per second of kernels_s), and the device alone at the big shape (skipped when 0).
--fractions: the counts are divided by each cell's size factor (counts per 10 000, what a normalised reference holds: fractional
values of full precision, the zeros kept), held as --dtype, and the device writer is called with fractions=True; the host path is
the fallback it replaces.  --pass-flag: the int64 frame, but fractions=True as save_results passes it.
One JSON line per leg; with --out they are appended to DIR/write_mtx_bench.jsonl."""
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

PHASES = ("narrow_s", "library_s", "upload_s", "kernels_s", "download_s", "write_s", "total_s")


def make_frame(G, N, density, seed, fractions=False, dtype="float64"):
    import pandas as pd
    rng = np.random.default_rng(seed)
    lam = -np.log1p(-density)                                # P(Poisson(lam) > 0) = density
    x = np.empty((G, N), np.int64)
    for g0 in range(0, G, 1000):
        x[g0:g0 + 1000] = rng.poisson(lam, (min(1000, G - g0), N))
    if fractions:
        x = (x * (1e4 / np.maximum(x.sum(axis=0), 1))).astype(dtype)
    return pd.DataFrame(x, index=[f"GENE_{i}" for i in range(G)], columns=[f"CELL_{i}" for i in range(N)], copy=False)


def host_path(path, frame, labels):
    """What save_results does for matrix.mtx without a device."""
    import scipy.io
    import scipy.sparse
    t = time.perf_counter()
    expr = frame.loc[:, labels]
    t1 = time.perf_counter()
    coo = scipy.sparse.coo_matrix(expr)
    t2 = time.perf_counter()
    scipy.io.mmwrite(path, coo)
    t3 = time.perf_counter()
    return {"gather_s": t1 - t, "coo_s": t2 - t1, "mmwrite_s": t3 - t2, "total_s": t3 - t}


def device_path(path, frame, labels, block_bytes, flag=False):
    from cytospace_amd.post_processing import write_mtx_device
    t = time.perf_counter()
    info = write_mtx_device(path, frame, frame.columns.get_indexer(labels), block_bytes=block_bytes, return_info=True,
                            **({"fractions": True} if flag else {}))
    info["call_s"] = time.perf_counter() - t                 # get_indexer included, as save_results pays it
    assert info["path"] == "device", info
    return info


def spread(ts):
    return {"min": round(min(ts), 4), "median": round(float(np.median(ts)), 4), "max": round(max(ts), 4), "n": len(ts)}


def medians(infos, keys):
    return {k: round(float(np.median([i[k] for i in infos])), 4) for k in keys}


def digest(path):
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as f:
        while True:
            b = f.read(64 << 20)
            if not b:
                return h.hexdigest()
            h.update(b)


def leg(G, N, C, density, reps, host_reps, block_bytes, d, seed, fractions=False, dtype="float64", flag=False):
    frame = make_frame(G, N, density, seed, fractions, dtype)
    labels = [f"CELL_{i}" for i in np.random.default_rng(seed + 1).integers(0, N, C)]
    pd_, ph_ = os.path.join(d, "device.mtx"), os.path.join(d, "host.mtx")
    dev, host = [], []
    for r in range(max(reps, host_reps)):                    # alternate the two paths
        if r < reps:
            dev.append(device_path(pd_, frame, labels, block_bytes, flag))
        if r < host_reps:
            host.append(host_path(ph_, frame, labels))
    out = {"genes": G, "cells": N, "assigned": C, "density": density, "dtype": str(frame.dtypes.iloc[0]), "fractions": fractions, "flag": flag, "nnz": dev[0]["nnz"], "bytes": dev[0]["bytes"],
           "blocks": dev[0]["blocks"], "field": dev[0]["field"], "device_s": spread([i["call_s"] for i in dev]),
           "device_phases": medians(dev, PHASES)}
    k = out["device_phases"]["kernels_s"]
    out["text_bytes_per_kernel_second"] = round(dev[0]["bytes"] / k) if k > 0 else None
    if host:
        out["host_s"] = spread([i["total_s"] for i in host])
        out["host_phases"] = medians(host, ("gather_s", "coo_s", "mmwrite_s"))
        out["speedup_median"] = round(out["host_s"]["median"] / out["device_s"]["median"], 2)
        out["equal"] = digest(pd_) == digest(ph_)
        assert out["equal"], "the device's file differs from the host's"
    for p in (pd_, ph_):
        if os.path.exists(p):
            os.remove(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=5000)
    ap.add_argument("--cells", type=int, default=8000)
    ap.add_argument("--assigned", type=int, default=20000)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--big-genes", type=int, default=0)
    ap.add_argument("--big-cells", type=int, default=0)
    ap.add_argument("--big-assigned", type=int, default=0)
    ap.add_argument("--big-reps", type=int, default=5)
    ap.add_argument("--big-host-reps", type=int, default=0)
    ap.add_argument("--block-bytes", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fractions", action="store_true", help="a fractional frame, written with fractions=True")
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"], help="the fractional frame's dtype")
    ap.add_argument("--pass-flag", action="store_true", help="fractions=True on the int64 frame")
    a = ap.parse_args()
    import ctypes
    from cytospace_amd import _lib
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().cyto_device_name(0, name, 256))
    d = tempfile.mkdtemp(prefix="write_mtx_bench_")
    lines = []
    try:
        kw = dict(fractions=a.fractions, dtype=a.dtype, flag=a.fractions or a.pass_flag)
        warm = leg(60, 300, 500, 0.1, 1, 1, 0, d, 7, **kw)  # warm-up: library, HIP, kernels, scipy's writer
        assert warm["equal"]
        legs = [(a.genes, a.cells, a.assigned, a.reps, a.host_reps, 0)]
        if a.big_genes and a.big_cells:
            legs.append((a.big_genes, a.big_cells, a.big_assigned or a.big_cells, a.big_reps, a.big_host_reps, 1))
        for G, N, C, reps, host_reps, seed in legs:
            res = dict(device=name.value.decode(), **leg(G, N, C, a.density, reps, host_reps, a.block_bytes, d, seed, **kw))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "write_mtx_bench.jsonl"), "a") as f:
            f.write("".join(l + "\n" for l in lines))


if __name__ == "__main__":
    main()
