"""The end of every batch of the several-searches-at-once kernel (wide_aug<.., PAR>) by parts, per workgroup.
Needs a -DCYTO_AUG_FIN_SPLIT build of the library (tools/build_variant.sh split -DCYTO_AUG_FIN_SPLIT), loaded through CYTOHIP_LIB.
usage: fin_split.py [u20000 u50000 ...] [--reps K] [--par K] [--batches] [--doomed]      (--batches: one line per batch of the last rep;
--doomed: per batch, how long it waited for searches that were then discarded -- last arrival less last committed arrival -- and the sum)

Per batch: the maximum over the workgroups of every part, and the parts of the batch's DEEPEST search (the last workgroup to reach the
end of its search: everybody else waits for it).  Per solve: the sums of both over the batches, in ms."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cytospace_amd import _lib  # noqa: E402
from cytospace_amd.lap import lap_solve  # noqa: E402
from tools import instances as I  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PARTS = ["claim", "wait1", "check", "wait2", "update", "walk", "cost", "reset", "wait3+log", "repair+bar4"]
WAITS = {"wait1", "wait2", "wait3+log"}
NTOUCH, SETTLED, HOPS, ARRIVE, ABORTED = 10, 11, 12, 13, 14


def dump():
    L = _lib.lib()
    if not hasattr(L, "cyto_wide_fin_split"):
        raise SystemExit("this library was not built with -DCYTO_AUG_FIN_SPLIT")
    mb, g, p = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.cyto_wide_fin_split(None, ctypes.byref(mb), ctypes.byref(g), ctypes.byref(p))
    out = np.zeros((mb.value, g.value, p.value), np.int64)
    rc = L.cyto_wide_fin_split(out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), ctypes.byref(mb), ctypes.byref(g), ctypes.byref(p))
    if rc:
        raise SystemExit(f"cyto_wide_fin_split: {rc}")
    return out


def main():
    tags = [a for a in sys.argv[1:] if not a.startswith("--") and not a.lstrip("-").isdigit()] or ["u20000"]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 2
    par = int(sys.argv[sys.argv.index("--par") + 1]) if "--par" in sys.argv else 0
    for tag in tags:
        n = int(np.load(os.path.join(GOLD, f"large_{tag}.npz"))["n"])
        if tag.startswith("u"):
            buf = I.blocks_to_device(I.uniform_cost_blocks(n), n)
        elif tag.startswith("t"):
            buf = I.blocks_to_device([(0, I.typed_unique_cost(n, n, 20)[0])], n)
        else:
            raise SystemExit(f"unknown tag {tag}")
        dump()                                                   # (clears what earlier solves left)
        for rep in range(reps):
            g = lap_solve(None, np.float32, return_info=True, device_ptr=buf.ptr, n=n, ld=n, opts=dict(mode=2, wide_par=par))
            inf = g["info"]
            d = dump()
            nb = int(inf.wide_par_batches)
            if nb <= 0 or nb > d.shape[0]:
                print(f"{tag} rep={rep}: {nb} batches: nothing recorded")
                continue
            d = d[:nb]
            t = d[:, :, :len(PARTS)].astype(np.float64) * 1e-5   # ms (100-MHz ticks)
            deep = np.argmax(d[:, :, ARRIVE], axis=1)            # per batch: the workgroup whose search ended last
            rows = np.arange(nb)
            mx, dp = t.max(axis=1), t[rows, deep]
            print(f"{tag} rep={rep}: aug={inf.ms_aug:.2f} ms, update+flip+reset timer {inf.wide_ms_aug_finish:.2f} ms, batches={nb} "
                  f"discarded={inf.wide_par_discarded}")
            print("    part          " + " ".join(f"{p:>11}" for p in PARTS))
            print("    sum of maxima " + " ".join(f"{x:11.3f}" for x in mx.sum(axis=0)))
            print("    deepest search" + " ".join(f"{x:11.3f}" for x in dp.sum(axis=0)))
            nw = [k for k, p in enumerate(PARTS) if p not in WAITS]
            print(f"    not waiting: sum of maxima {mx[:, nw].sum():.3f} ms, deepest searches (the critical path) {dp[:, nw].sum():.3f} ms; "
                  f"of that without repair+bar4 {dp[:, nw[:-1]].sum():.3f} ms")
            print(f"    deepest searches: ntouch {int(d[rows, deep, NTOUCH].sum())} (largest {int(d[rows, deep, NTOUCH].max())}), "
                  f"settled {int(d[rows, deep, SETTLED].sum())} (largest {int(d[rows, deep, SETTLED].max())}), "
                  f"path hops {int(d[rows, deep, HOPS].sum())} (longest {int(d[rows, deep, HOPS].max())}); "
                  f"all searches: ntouch {int(d[:, :, NTOUCH].sum())} settled {int(d[:, :, SETTLED].sum())}")
            if "--doomed" in sys.argv:
                # what a batch waits for searches that are then discarded: the last arrival of all its searches less the last arrival
                # of a committed one (a committed search has flipped a path: hops > 0).  The sum over the batches is the most that
                # ending doomed searches early can take off the solve.
                arr = d[:, :, ARRIVE]
                com = d[:, :, HOPS] > 0
                last_all = arr.max(axis=1)
                last_com = np.where(com, arr, 0).max(axis=1)
                ok = com.any(axis=1)
                gap = np.where(ok, last_all - last_com, 0) * 1e-2                           # us
                # (a library with the early end of doomed searches records which searches it aborted: part 14)
                ab = d[:, :, ABORTED] > 0 if d.shape[2] > ABORTED else np.zeros(arr.shape, bool)
                print(f"    aborted searches: {int(ab.sum())} of {int(inf.wide_par_discarded)} discarded")
                print(f"    doomed: sum over batches of (last arrival - last committed arrival) {gap.sum() * 1e-3:.3f} ms, "
                      f"largest {gap.max():.1f} us in batch {int(gap.argmax())}, batches with a gap {int((gap > 0).sum())} of {nb}"
                      + ("" if ok.all() else f"; {int((~ok).sum())} batches without a committed search left out"))
                if rep == reps - 1:
                    for b in range(nb):
                        print(f"    batch {b:4d} committed={int(com[b].sum()):2d} aborted={int(ab[b].sum()):2d} last g={int(deep[b]):2d} "
                              f"last committed g={int(np.where(com[b], arr[b], 0).argmax()):2d} gap={gap[b]:8.1f} us")
            if "--batches" in sys.argv and rep == reps - 1:
                for b in range(nb):
                    print(f"    batch {b:4d} deepest g={int(deep[b]):2d} ntouch={int(d[b, deep[b], NTOUCH]):6d} settled={int(d[b, deep[b], SETTLED]):6d} "
                          f"hops={int(d[b, deep[b], HOPS]):4d} us: " + " ".join(f"{x * 1e3:7.1f}" for x in dp[b]) + " | max: "
                          + " ".join(f"{x * 1e3:7.1f}" for x in mx[b]))
        buf.free()


if __name__ == "__main__":
    main()
