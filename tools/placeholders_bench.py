"""place_holders_device against the host loop of sample_single_cells' "place_holders" branch at a production size.

  python tools/placeholders_bench.py [--genes 15000] [--cells 300] [--short 5000] [--out DIR]      GPU: one JSON line

A cell type of `cells` cells that needs cells + short: `short` synthetic cells of `genes` genes, genes * short draws (int64
counts, Poisson).  The device call is timed with a host clock around the whole of it (upload, kernels, download), after a small
warm-up call, and repeated; its result is compared, with numpy's state afterwards, against ONE np.random.randint(0, n, (short,
genes)) and a numpy gather -- what the host loop computes (tests/test_placeholders_cpu.py) and the only form of it that ends
at this size.  The loop itself (one np.random.choice per draw) is run at short = 5, compared as well, and its time is
SCALED linearly to `short`: the record says so."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def same_state(a, b):
    return bool(a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:])


def bench(G, n, short, repeats=3, loop_short=5):
    from cytospace_amd import _lib
    from cytospace_amd.common import place_holders_device
    from cytospace_amd.cytospace import _place_holders_host
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().cyto_device_name(0, name, 256))
    own = np.random.default_rng(0).poisson(2.0, (G, n)).astype(np.int64)
    np.random.seed(0)
    place_holders_device(own[:200], 70)                                   # warm-up: library, HIP, kernels

    times = []
    for _ in range(repeats):
        np.random.seed(1)
        (dev, words), t = timed(lambda: place_holders_device(own, short, return_words=True))
        times.append(t)
    s_dev = np.random.get_state()
    np.random.seed(1)
    idx, t_randint = timed(lambda: np.random.randint(0, n, size=(short, G)))
    s_host = np.random.get_state()
    equal = same_state(s_dev, s_host) and bool(np.array_equal(dev, own[np.arange(G)[:, None], idx.T].astype(np.float64)))
    del idx

    np.random.seed(1)
    loop, t_loop = timed(lambda: _place_holders_host(own, loop_short))
    s_loop = np.random.get_state()
    np.random.seed(1)
    dev5 = place_holders_device(own, loop_short)
    equal_loop = same_state(np.random.get_state(), s_loop) and bool(np.array_equal(dev5, loop))
    draws = G * short
    dev_s = min(times)
    return {"device": name.value.decode(), "genes": G, "cells": n, "short": short, "draws": draws, "words": int(words),
            "device_s": round(dev_s, 4), "device_s_all": [round(t, 4) for t in times],
            "device_words_per_s": round(words / dev_s), "equal": equal,
            "host_loop": {"short": loop_short, "seconds": round(t_loop, 3), "us_per_draw": round(t_loop / (G * loop_short) * 1e6, 2),
                          "equal": equal_loop},
            "host_s_scaled": round(t_loop * short / loop_short, 1), "host_s_is_scaled_from_short": loop_short,
            "speedup_vs_scaled_host": round(t_loop * short / loop_short / dev_s, 1),
            "numpy_randint_alone_s": round(t_randint, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=15000)
    ap.add_argument("--cells", type=int, default=300)
    ap.add_argument("--short", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(bench(a.genes, a.cells, a.short, a.repeats))
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "placeholders_bench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
