"""estimate_cell_number_RNA_reads: the column sums on the device against the form it replaced, at production sizes.

  python tools/cells_per_spot_bench.py [--genes 20000] [--spots 5000 20000] [--runs 5] [--out DIR]      GPU: one JSON line per shape

The ST table is an int64 DataFrame of Poisson counts.  Two forms of the same function are timed with a host clock around the whole
call, alternating, after one warm-up of each:

  parent   reads = normalize_data(st.values.astype(float)).sum(axis=0, dtype=float), then the polyfit tail -- the float64 matrix goes
           up, the normalised float64 matrix comes back and numpy adds it up
  new      cytospace.estimate_cell_number_RNA_reads: the counts go up in their narrowest dtype, S doubles come back

Both results are compared (they must be equal).  Also recorded: the summing kernel's own HIP-event time (median of the runs), and
the call on a resident.DeviceFrame of the same table (no upload at all)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def parent_estimate(st_data, mean_cell_numbers, device_id=0):
    """estimate_cell_number_RNA_reads as it was before the sums moved to the device."""
    from cytospace_amd import common
    reads = common.normalize_data(st_data.values.astype(float), device_id).sum(axis=0, dtype=float)
    lo, mid = reads.min(), reads.mean()
    line = np.poly1d(np.polyfit(np.array([lo, mid]), np.array([1 if lo > 0 else 0, mean_cell_numbers]), 1))
    return line(reads).astype(int)


def spread(ts):
    return {"median_s": round(statistics.median(ts), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
            "all_s": [round(t, 4) for t in ts]}


def bench(G, S, runs):
    import pandas as pd
    from cytospace_amd import _lib, common
    from cytospace_amd.cytospace import estimate_cell_number_RNA_reads
    from cytospace_amd.resident import DeviceFrame
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().cyto_device_name(0, name, 256))
    st = pd.DataFrame(np.random.default_rng(S).poisson(1.0, (G, S)).astype(np.int64))
    want = parent_estimate(st, 5)                                            # warm-up of both forms at this shape
    equal = bool(np.array_equal(estimate_cell_number_RNA_reads(st, 5), want))
    t_parent, t_new, t_frame, k_ms = [], [], [], []
    for _ in range(runs):
        r, t = timed(lambda: parent_estimate(st, 5))
        t_parent.append(t)
        equal = equal and bool(np.array_equal(r, want))
        r, t = timed(lambda: estimate_cell_number_RNA_reads(st, 5))
        t_new.append(t)
        equal = equal and bool(np.array_equal(r, want))
    frame = DeviceFrame.from_frame(st)
    try:
        estimate_cell_number_RNA_reads(frame, 5)
        for _ in range(runs):
            r, t = timed(lambda: estimate_cell_number_RNA_reads(frame, 5))
            t_frame.append(t)
            equal = equal and bool(np.array_equal(r, want))
        fetches = frame.fetches
    finally:
        frame.close()
    x = np.ascontiguousarray(st.values, dtype=np.uint8)
    for _ in range(runs):
        k_ms.append(common.normalized_column_sums(x, return_kernel_ms=True)[1])
    mp, mn = statistics.median(t_parent), statistics.median(t_new)
    return {"device": name.value.decode(), "genes": G, "spots": S, "runs": runs, "equal": equal,
            "parent": spread(t_parent), "new": spread(t_new), "new_on_device_frame": spread(t_frame), "frame_fetches": fetches,
            "kernel_ms_median": round(statistics.median(k_ms), 3), "kernel_ms_all": [round(v, 3) for v in k_ms],
            "parent_over_new": round(mp / mn, 2),
            "new_below_parent_by_more_than_the_spread": bool(max(t_new) < min(t_parent))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--spots", type=int, nargs="+", default=[5000, 20000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for S in a.spots:
        line = json.dumps(bench(a.genes, S, a.runs))
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "cells_per_spot_bench.jsonl"), "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
