"""Wide solver at true sizes against the committed goldens (colsol; spot level where rows are duplicated) + timing.
usage: wide_large.py [u20000 u50000 c3s50000 c4s10000 t20000 ...] [--chain] [--rounds R] [--par K | --par -1] [--rebuild K | --rebuild -1] [--reps K]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cytospace_amd.lap import lap_solve, lap_solve_rows  # noqa: E402
from tools import instances as I  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    tags = [a for a in sys.argv[1:] if not a.startswith("--") and not a.lstrip("-").isdigit()] or ["u20000"]
    mode = 1 if "--chain" in sys.argv else 2
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 0
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 2
    rebuild = int(sys.argv[sys.argv.index("--rebuild") + 1]) if "--rebuild" in sys.argv else 0
    par = int(sys.argv[sys.argv.index("--par") + 1]) if "--par" in sys.argv else 0
    for tag in tags:
        d = np.load(os.path.join(GOLD, f"large_{tag}.npz"))
        n = int(d["n"])
        loc = None
        if tag.startswith("u"):
            buf = I.blocks_to_device(I.uniform_cost_blocks(n), n)
        elif tag.startswith("c3s"):
            uniq, loc = I.c3_shaped_unique(n)
            buf = I.blocks_to_device(I.repeated_row_blocks(uniq, loc), n)
        elif tag.startswith("c4s"):
            c, loc = I.c4_chunk_cost(n)
            buf = I.blocks_to_device([(0, c)], n)
        elif tag.startswith("t"):
            buf = I.blocks_to_device([(0, I.typed_unique_cost(n, n, 20)[0])], n)
        else:
            raise SystemExit(f"unknown tag {tag}")
        for rep in range(reps):
            t = time.time()
            g = lap_solve(None, np.float32, return_info=True, device_ptr=buf.ptr, n=n, ld=n, opts=dict(mode=mode, wide_rounds=rounds, wide_rebuild=rebuild, wide_par=par))
            wall = time.time() - t
            inf = g["info"]
            same = np.array_equal(g["colsol"], d["colsol"])
            # the wide restatement's golden: duals and row solution by their hashes (a schedule-dependent kernel shows here first)
            wpath = os.path.join(GOLD, f"large_{tag}_wide.npz")
            duals = "n/a"
            if mode == 2 and rounds == 0 and os.path.exists(wpath):
                import hashlib
                dw = np.load(wpath)
                duals = all(hashlib.sha256(np.ascontiguousarray(g[k]).tobytes()).hexdigest() == str(dw[k + "_sha256"]) for k in ("u", "v", "rowsol"))
            spot = same if loc is None else np.array_equal(loc[g["colsol"]], loc[d["colsol"]])
            print(f"{tag} mode={mode} rep={rep}: colsol==golden {same} duals==wide-golden {duals} spot-level {spot} total diff {g['total'] - float(d['total']):.3e} "
                  f"ms colred={inf.ms_colred:.2f} cache={inf.ms_cache:.2f} arr={inf.ms_arr:.2f} aug={inf.ms_aug:.2f} total={inf.ms_total:.2f} wall={wall * 1e3:.1f} | "
                  f"free={inf.free_after_arr2} rounds={inf.wide_rounds} bids={inf.scans_arr} retired={inf.wide_retired} relax={inf.scans_aug_relax} "
                  f"settled={inf.wide_aug_settled} aug_rounds={inf.wide_aug_rounds} dense=({inf.wide_dense_arr},{inf.wide_dense_aug}) launches={inf.wide_aug_launches} "
                  f"trivial={inf.wide_trivial} verify={inf.wide_verify_passes} hops={inf.path_hops} par_batches={inf.wide_par_batches} discarded={inf.wide_par_discarded}", flush=True)
            from cytospace_amd import _lib
            if hasattr(_lib.lib(), "cyto_wide_embedded_solves"):      # (a process-wide count: grows by one per solve whose searches ran embedded)
                print(f"    embedded solves so far: {_lib.wide_embedded_solves()}", flush=True)
            print(f"    wide_arr: list rounds {inf.wide_list_rounds} ({inf.wide_ms_list:.2f} ms), chain rounds {inf.wide_chain_rounds} ({inf.wide_ms_chain:.2f} ms) | "
                  f"wide_aug: rounds {inf.wide_ms_aug_rounds:.2f} ms, certificate passes {inf.wide_ms_aug_verify:.2f}, update+flip+reset {inf.wide_ms_aug_finish:.2f}, "
                  f"one-edge searches {inf.wide_ms_aug_trivial:.2f}", flush=True)
        buf.free()


if __name__ == "__main__":
    main()
