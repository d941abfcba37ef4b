"""What cyto_lap_opts.exact costs: the same device-resident instances solved plain, with certify = 1, exact = 1 and polish = 1
("Exact option").

  python tools/exact_cost_bench.py [--reps 3] [--skip-large]      GPU: one JSON line per leg

Legs: uniform 50 000^2 (SURVEY 8d's instance), few-cell-type 20 000^2 (tools/instances.typed_unique_cost, K = 5), 256 chunk LAPs
of 10 000^2 in one batched call (bench.py's c4_chunks instances; a batch has no polish), and instance 283 of
tests/golden/cross_unique.npz (the known near-tie).  Per mode: the median host wall time of `reps` solves after one warm-up, the
solver's kernel time, and the exact option's own counters."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"plain": None, "certify": dict(certify=1), "exact": dict(exact=1), "polish": dict(polish=1)}


def _info(i):
    return {"kernel_ms": round(i.ms_total, 2), "gap_rows": int(i.gap_rows), "exact_status": int(i.exact_status),
            "exact_edges": int(i.exact_edges), "exact_changed_rows": int(i.exact_changed_rows),
            "exact_overflow_rows": int(i.exact_overflow_rows), "exact_ms_emit": round(i.exact_ms_emit, 3),
            "exact_ms_repair": round(i.exact_ms_repair, 3), "polished": int(i.polished), "polish_ms": round(i.polish_ms, 2)}


def single(name, solve, reps, modes):
    out = {"leg": name}
    for m in modes:
        solve(MODES[m])
        walls, last = [], None
        for _ in range(reps):
            t = time.perf_counter()
            last = solve(MODES[m])
            walls.append(time.perf_counter() - t)
        out[m] = dict(wall_ms=round(1e3 * float(np.median(walls)), 2), **_info(last["info"]))
    for m in modes:
        if m != "plain":
            out[m]["over_plain_ms"] = round(out[m]["wall_ms"] - out["plain"]["wall_ms"], 2)
    print(json.dumps(out), flush=True)
    return out


def main():
    from cytospace_amd.lap import lap_solve, lap_solve_batch_device
    from cytospace_amd import _lib
    from tools import cross_unique, instances
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    dev = 0
    c = cross_unique.instance("typed", 2973, 5283, 4)
    single("i283_typed_2973", lambda o: lap_solve(c, np.float32, return_info=True, opts=o), reps, list(MODES))
    if "--skip-large" not in sys.argv:
        n = 50000
        buf = instances.blocks_to_device(instances.uniform_cost_blocks(n), n, dev)
        single("uniform_50000", lambda o: lap_solve(None, np.float32, return_info=True, device_ptr=buf.ptr, n=n, ld=n, opts=o), reps,
               list(MODES))
        buf.free()
        n = 20000
        t = instances.typed_unique_cost(n, n, 20000, K=5)[0]
        buf = _lib.DeviceBuffer.from_numpy(t, dev)
        del t
        single("typed5_20000", lambda o: lap_solve(None, np.float32, return_info=True, device_ptr=buf.ptr, n=n, ld=n, opts=o), reps,
               list(MODES))
        buf.free()
    # 256 chunk LAPs in one batched call (4 distinct instances, every problem its own copy)
    n, K, distinct = 10000, 256, 4
    bufs = [_lib.DeviceBuffer.from_numpy(instances.c4_chunk_cost(n, seed=4 + k)[0], dev) for k in range(distinct)]
    bufs += [bufs[k % distinct].clone() for k in range(distinct, K)]

    def batch(o):
        res = lap_solve_batch_device([b.ptr for b in bufs], [n] * K, device_id=dev, max_concurrent=K, return_info=True, opts=o)
        r0 = dict(res[0])
        r0["info"] = res[int(np.argmax([r["info"].exact_changed_rows for r in res]))]["info"]
        return r0
    single("batch_256x10000", batch, max(2, reps - 1), ["plain", "certify", "exact"])
    for b in bufs:
        b.free()


if __name__ == "__main__":
    main()
