"""The classic true-size goldens through cyto_lap_opts.exact: every uniqueness-certified answer must come back whatever build of the
solver runs (CYTOHIP_LIB=<a variant build, e.g. tools/build_variant.sh stop128 -DWIDE_STOP_CAP=128>).

  python tools/exact_goldens.py [tag ...]      GPU: one JSON line per golden, then a summary line; exit status 1 on a mismatch"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

TAGS = ["t10000", "t20000", "t30000", "k5t20000", "c4s10000", "c4s16384", "u20000", "u50000"]


def main(tags):
    import make_golden_large as mg
    from cytospace_amd import _lib
    from cytospace_amd.lap import lap_solve
    from tools import instances
    bad = 0
    for tag in tags:
        d = np.load(os.path.join(ROOT, "tests", "golden", f"large_{tag}.npz"))
        t = time.perf_counter()
        if tag.startswith("u"):
            n, loc = int(tag[1:]), None
            buf = instances.blocks_to_device(instances.uniform_cost_blocks(n), n)
        else:
            n, cost, loc = mg.instance(tag)
            buf = _lib.DeviceBuffer.from_numpy(np.ascontiguousarray(cost, np.float32), 0)
            del cost
        gen = time.perf_counter() - t
        g = lap_solve(None, np.float32, return_info=True, device_ptr=buf.ptr, n=n, ld=n, opts=dict(exact=1))
        buf.free()
        i = g["info"]
        same = bool(np.array_equal(g["colsol"], d["colsol"]) if loc is None else np.array_equal(loc[g["colsol"]], loc[d["colsol"]]))
        bad += not same
        print(json.dumps({"tag": tag, "n": n, "golden_indices": same, "gap_f64": i.gap_f64, "gap_rows": int(i.gap_rows),
                          "exact_status": int(i.exact_status), "exact_edges": int(i.exact_edges),
                          "exact_changed_rows": int(i.exact_changed_rows), "exact_ms_emit": round(i.exact_ms_emit, 3),
                          "exact_ms_repair": round(i.exact_ms_repair, 3), "solve_ms": round(i.ms_total, 1), "gen_s": round(gen, 1),
                          "lib": os.path.basename(_lib.LIB_PATH)}), flush=True)
    print(json.dumps({"goldens": len(tags), "mismatches": bad}), flush=True)
    return bad


if __name__ == "__main__":
    sys.exit(1 if main(sys.argv[1:] or TAGS) else 0)
