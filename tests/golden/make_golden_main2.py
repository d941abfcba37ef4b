"""gv15: whole runs of the reference's main_cytospace on the paths gv14's five runs never take -- the other two metrics, 10x
MatrixMarket directories (integer and real), tab-separated tables, place-holders in single-cell mode, a cell type short of cells
under `duplicates` (repeated cells: exact ties), a result with as many cells as genes, an output prefix, and two runs beyond toy
size (one LAP of several hundred rows; estimated cell numbers feeding sub-spot chunks).

Run here (imports /root/reference read-only).  Like gv14 the fixture holds the INPUT files and the OUTPUT files' bytes of every
run plus its arguments -- no reference source -- in gv14's key layout (`tag::args`, `tag::in::<path>`, `tag::out::<path>`), split
over two files (FILES) so that each stays below the largest fixture committed before it.  inputs(), the exact solver and the stub
modules are make_golden_main.py's; the pandas reader replaces the reference's read_file for delimited text only: a path ending in
`.mtx` goes through the reference's own read_file (scipy).

Stability: as in gv14 a run is rejected (the generator fails; move to the next seed) if any of its LAPs gives another spot-level
answer when the cost is rounded to float32.  Here the note of such a LAP goes through a file, so that the chunks the reference
solves in forked workers are seen too (a list in this process, gv14's way, never hears of them).  `duplicates_short` holds
identical columns, which an exact solver may swap; it is run twice instead, on the float64 cost and on the float32-rounded one,
and the two assigned_locations.csv must be equal as multisets of rows without the UniqueCID column.  The partitioned runs
(ROW_SETS) draw some cells twice as well -- 900 cells for about 1 000 slots -- and a chunk that receives both copies swaps them at
will (seed 27 does so in one chunk, and gv14's rule flags seeds 28 to 35 too); the test compares those runs as sets of rows without UniqueCID, so for them the rule is applied
with identical cells taken together (noting_solver).  Every run compared byte for byte keeps gv14's rule as it is.

Run:  python tests/golden/make_golden_main2.py
"""
import io
import json
import os
import sys
import tempfile

import numpy as np
import pandas as pd
import scipy.io
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_main import COMMON, inputs, pandas_read_file, ref  # noqa: E402  (stubs, reference path, swapped solver)
from make_golden import exact_solver_lapjv_shape  # noqa: E402
import cytospace.common as ref_common  # noqa: E402

FILES = ("gv15_main.npz", "gv15_main_large.npz")
LARGE = ("larger", "larger_estimated_subspots")         # the runs of the second file
ROW_SETS = ("single_cell_placeholders", "larger_estimated_subspots")    # partitioned runs: the test compares them as sets of rows
CAP = 621726                                            # gv5_solve_lap.npz, the largest fixture committed before gv15
NOTES = None                                            # path of the file every solved LAP is noted in (forked workers append too)
ROUND = "check"                                         # "check": gv14's rule; "f64" / "f32": solve that cost, check nothing


def read_file(path):
    return ref_common.read_file(path) if path.endswith(".mtx") else pandas_read_file(path)


def _classes(vectors):
    """A class number per vector: equal up to the reference's 1e-16 noise (rounded to 1e-9; a value on a rounding edge can only
    split a class, which makes the check stricter)."""
    seen = {}
    return [seen.setdefault(tuple(np.round(v, 9)), len(seen)) for v in vectors]


def noting_solver(cost):
    """make_golden_main's spot_level_solver with its note written to NOTES, one line per LAP: `rows columns moved moved_sets`.
    moved: gv14's rule -- some cell's spot differs between the float64 cost and the float32-rounded one.  moved_sets: the same
    with identical cells (equal cost columns: a cell drawn twice) taken together -- the multiset of their spots differs.  Equal
    cells are interchangeable to an exact solver, so `moved` without `moved_sets` is a swap that only the UniqueCID column shows."""
    cost = np.asarray(cost, dtype=np.float64)
    c32 = cost.astype(np.float32).astype(np.float64)
    moved = moved_sets = 0
    if ROUND == "f32":
        a = exact_solver_lapjv_shape(c32)
    else:
        a = exact_solver_lapjv_shape(cost)
        if ROUND == "check":
            b = exact_solver_lapjv_shape(c32)
            # rows are spot slots: two rows are the same spot iff their cost rows agree up to the reference's 1e-16 noise
            moved = int(not all(np.abs(cost[a[1][j]] - cost[b[1][j]]).max() < 1e-12 for j in range(cost.shape[1])))
            spot, cell = _classes(cost), _classes(cost.T)
            sets = lambda sol: sorted((cell[j], spot[sol[1][j]]) for j in range(cost.shape[1]))   # noqa: E731
            moved_sets = int(sets(a) != sets(b))
    with open(NOTES, "a") as f:
        f.write(f"{cost.shape[0]} {cost.shape[1]} {moved} {moved_sets}\n")
    return a


ref.read_file = read_file
ref.import_solver = lambda method: noting_solver


# ---- how a run's tables reach the disk: each returns the path arguments that differ from gv14's ----

def as_csv(files):
    for name, df in files.items():
        df.to_csv(name)
    return {}


def as_tab(files):
    files = dict(files)
    files.pop("scRNA.csv").to_csv("scRNA.tsv", sep="\t")
    files.pop("st.csv").to_csv("st.txt", sep="\t")
    as_csv(files)
    return dict(scRNA_path="scRNA.tsv", st_path="st.txt")


def _tenx(folder, df, values, gene_file, cell_file):
    """A 10x directory: matrix.mtx in coordinate form with the gene and cell lists beside it (no header; a .tsv list carries
    the id twice, as Cell Ranger's genes.tsv does)."""
    os.makedirs(folder)
    scipy.io.mmwrite(os.path.join(folder, "matrix.mtx"), scipy.sparse.coo_matrix(values))
    for name, labels in ((gene_file, df.index), (cell_file, df.columns)):
        cols = [list(labels)] * (2 if name.endswith(".tsv") else 1)
        pd.DataFrame(dict(enumerate(cols))).to_csv(os.path.join(folder, name), sep="\t" if name.endswith(".tsv") else ",",
                                                   header=False, index=False)


def as_mtx_integer(files):
    files = dict(files)
    sc, st = files.pop("scRNA.csv"), files.pop("st.csv")
    _tenx("sc10x", sc, sc.to_numpy(), "genes.tsv", "barcodes.tsv")
    _tenx("st10x", st, st.to_numpy(), "features.tsv", "cells.csv")
    as_csv(files)
    return dict(scRNA_path="sc10x/matrix.mtx", st_path="st10x/matrix.mtx")


def as_mtx_real(files):
    files = dict(files)
    sc, st = files.pop("scRNA.csv"), files.pop("st.csv")
    _tenx("sc10x", sc, sc.to_numpy().astype(np.float64), "genes.tsv", "barcodes.tsv")         # whole numbers, `real` field
    _tenx("st10x", st, st.to_numpy() / 4, "features.tsv", "cells.csv")                        # quarters: exact in binary
    as_csv(files)
    return dict(scRNA_path="sc10x/matrix.mtx", st_path="st10x/matrix.mtx")


def as_square(files):
    files = dict(files)
    n = files["ncells.csv"]
    files["ncells.csv"] = pd.DataFrame({"Number of cells": [4] * 12 + [5] * 8}, index=n.index)   # 88 cells: the genes scRNA keeps
    return as_csv(files)


BOTH = dict(n_cells_per_spot_path="ncells.csv", cell_type_fraction_estimation_path="fractions.csv")
RUNS = {
    # tag: (inputs' seed, inputs' shape, how the tables are written, arguments beyond gv14's common ones)
    "spearman": (21, {}, as_csv, dict(BOTH, distance_metric="Spearman_correlation")),
    "euclidean": (22, {}, as_csv, dict(BOTH, distance_metric="Euclidean")),
    "mtx_integer": (23, {}, as_mtx_integer, dict(BOTH)),
    "mtx_real": (41, {}, as_mtx_real, dict(BOTH, downsample_off=True)),
    "tab_separated": (42, {}, as_tab, dict(BOTH)),
    "single_cell_placeholders": (24, dict(single=True, C=30), as_csv,
                                 dict(n_cells_per_spot_path=None, cell_type_fraction_estimation_path="fractions.csv", single_cell=True,
                                      number_of_selected_spots=9, sampling_method="place_holders")),
    "duplicates_short": (31, dict(C=36), as_csv, dict(BOTH)),
    "square_result": (43, {}, as_square, dict(BOTH)),
    "larger": (25, dict(G=300, C=1500, S=300), as_csv, dict(BOTH, seed=11)),
    "larger_estimated_subspots": (27, dict(G=200, C=900, S=200), as_csv,
                                  dict(n_cells_per_spot_path=None, cell_type_fraction_estimation_path="fractions.csv",
                                       sampling_sub_spots=True, number_of_selected_sub_spots=150, seed=7, output_prefix="run_")),
}


def tree(top):
    out = {}
    for root, _, fs in os.walk(top):
        for f in sorted(fs):
            path = os.path.join(root, f)
            out[os.path.relpath(path, top)] = open(path, "rb").read()
    return out


def run_reference(args, how, folder="out"):
    """One run of the reference in the working directory; returns (output files, the LAPs' notes)."""
    global NOTES, ROUND
    ROUND = how
    args = dict(args, output_folder=folder)
    fd, NOTES = tempfile.mkstemp(suffix=".laps")
    os.close(fd)
    try:
        ref.main_cytospace(**args)
        laps = [tuple(map(int, ln.split())) for ln in open(NOTES)]
    finally:
        os.remove(NOTES)
    return tree(args["output_folder"]), laps


def assigned_rows(text):
    df = pd.read_csv(io.StringIO(text.decode())).drop(columns="UniqueCID")
    return sorted(map(tuple, df.astype(str).to_numpy().tolist()))


def main():
    gv = [{}, {}]
    cwd = os.getcwd()
    for tag, (seed, shape, write, kw) in RUNS.items():
        part = gv[tag in LARGE]
        with tempfile.TemporaryDirectory() as d:
            os.chdir(d)
            try:
                paths = write(inputs(seed, **shape))
                for rel, data in tree(".").items():
                    part[f"{tag}::in::{rel}"] = np.frombuffer(data, dtype=np.uint8)
                args = dict(scRNA_path="scRNA.csv", cell_type_path="cell_types.csv", st_path="st.csv", coordinates_path="coords.csv",
                            st_cell_type_path=None, output_folder="out", **COMMON)
                args.update(kw)
                args.update(paths)
                prefix = args.get("output_prefix", "")
                if tag == "duplicates_short":
                    out, laps = run_reference(args, "f64")
                    out32, _ = run_reference(args, "f32", "out32")
                    name = "assigned_locations.csv"
                    if assigned_rows(out[name]) != assigned_rows(out32[name]):
                        raise SystemExit(f"{tag}: the float32-rounded cost assigns another multiset of (cell, spot) rows; change the seed")
                    ids = pd.read_csv(io.BytesIO(out[name])).OriginalCID
                    if not ids.duplicated().any():
                        raise SystemExit(f"{tag}: no cell is assigned twice; change the seed")
                    print(f"  {tag}: {len(ids)} cells assigned, {ids.nunique()} distinct; float64 and float32 runs "
                          f"{'byte-equal' if out[name] == out32[name] else 'multiset-equal only'}")
                else:
                    out, laps = run_reference(args, "check")
                    bad = [l[:2] for l in laps if l[3 if tag in ROW_SETS else 2]]
                    if bad:
                        raise SystemExit(f"{tag}: spot-level answer changes in float32 for LAPs {bad}; change the seed")
                    if any(l[2] for l in laps):
                        print(f"  {tag}: {sum(l[2] for l in laps)} LAP(s) swap identical cells between the two costs")
                if tag == "square_result":
                    m = scipy.io.mmread(io.BytesIO(out["assigned_expression/matrix.mtx"]))
                    if m.shape[0] != m.shape[1]:
                        raise SystemExit(f"{tag}: the reference wrote {m.shape[0]} genes x {m.shape[1]} cells, not a square")
                if tag == "single_cell_placeholders" and pd.read_csv(io.BytesIO(out["new_scRNA.csv"]), index_col=0).shape[1] == 0:
                    raise SystemExit(f"{tag}: no cell type is short of cells; change the seed")
                if tag == "larger" and (len(laps) != 1 or laps[0][0] < 300):
                    raise SystemExit(f"{tag}: one LAP of at least 300 rows is wanted, got {laps}")
                part[f"{tag}::args"] = np.frombuffer(json.dumps(args).encode(), dtype=np.uint8)
                for rel, data in out.items():
                    part[f"{tag}::out::{rel}"] = np.frombuffer(data, dtype=np.uint8)
                print(f"  {tag}: LAP rows {sorted(l[0] for l in laps)}, {len(out)} output files (prefix {prefix!r})")
            finally:
                os.chdir(cwd)
    for name, part in zip(FILES, gv):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        size = os.path.getsize(path)
        print(f"gv15: {name}: {len({k.split('::')[0] for k in part})} runs, {len(part)} entries, {size} bytes")
        if size > CAP:
            raise SystemExit(f"{name} is larger than {CAP} bytes: shrink larger_estimated_subspots")


if __name__ == "__main__":
    main()
