"""gv14: whole runs of the reference's main_cytospace (cytospace/cytospace.py:472-717) on small synthetic inputs.

Run here (imports /root/reference read-only).  The fixture holds the INPUT files and the OUTPUT files' bytes of every run, plus its
arguments -- no reference source.  Absent third-party modules are stubbed as in make_golden_outputs.py; the reference's
read_file (datatable) is swapped for a pandas reader of the same tables, import_solver for an exact solver with lapjv's return
shape, and plots are off.  An instance is rejected (and the generator fails) if any of its LAPs gives a different spot-level
answer when the cost is rounded to float32, so that the float32 GPU solver is expected to reproduce it.
gv15 (make_golden_main2.py) reuses inputs(), the solver and the stubs from here for the runs these five leave out: the other
metrics, MatrixMarket and tab-separated inputs, repeated cells, a square result, an output prefix and sizes beyond toys.

Run:  python tests/golden/make_golden_main.py
"""
import json
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_outputs  # noqa: E402,F401  (installs the stub modules and the reference path)
from make_golden import exact_solver_lapjv_shape  # noqa: E402
import cytospace.cytospace as ref  # noqa: E402

OUT = os.path.join(HERE, "gv14_main.npz")
UNSTABLE = []


def pandas_read_file(path):
    return pd.read_csv(path, sep="," if path.lower().endswith(".csv") else "\t", header=0, index_col=0)


def spot_level_solver(cost):
    """Exact solve; records an instance whose spot-level answer moves when the cost is rounded to float32."""
    cost = np.asarray(cost, dtype=np.float64)
    a = exact_solver_lapjv_shape(cost)
    b = exact_solver_lapjv_shape(cost.astype(np.float32).astype(np.float64))
    # rows are spot slots: two rows are the same spot iff their cost rows agree up to the reference's 1e-16 noise
    if not all(np.abs(cost[a[1][j]] - cost[b[1][j]]).max() < 1e-12 for j in range(cost.shape[1])):
        UNSTABLE.append(cost.shape)
    return a


ref.read_file = pandas_read_file
ref.import_solver = lambda method: spot_level_solver


def inputs(seed, G=90, C=150, S=20, K=3, single=False):
    rng = np.random.default_rng(seed)
    base = rng.lognormal(0, 1.2, G)
    prof = rng.lognormal(0, 1.0, (K, G)) * base
    ctype = rng.integers(0, K, C)
    depth = rng.integers(60, 400, C)
    sc = np.stack([rng.multinomial(depth[c], prof[ctype[c]] / prof[ctype[c]].sum()) for c in range(C)], axis=1)
    ncells = np.ones(S, np.int64) if single else rng.integers(1, 4, S)
    st_type = rng.integers(0, K, S)
    st = np.zeros((G, S), np.int64)
    for s in range(S):
        mix = rng.dirichlet(np.ones(K)) if not single else np.eye(K)[st_type[s]]
        p = (mix @ prof) / (mix @ prof).sum()
        st[:, s] = rng.multinomial(int(250 * ncells[s]), p)
    genes = [f"G{i}" for i in range(G)]
    genes[5] = genes[4]                                            # a duplicated gene: dropped by read_data
    names = ["Bcell", "Tcell", "Mono"]
    files = {
        "scRNA.csv": pd.DataFrame(sc, index=genes, columns=[f"c{i}" for i in range(C)]),
        "cell_types.csv": pd.DataFrame({"CellType": [names[t] for t in ctype]}, index=[f"c{i}" for i in range(C)]),
        "st.csv": pd.DataFrame(st, index=genes[:G - 3] + ["X1", "X2", "X3"], columns=[f"s{i}" for i in range(S)]),
        "coords.csv": pd.DataFrame({"row": np.arange(S) // 6, "col": np.arange(S) % 6}, index=[f"s{i}" for i in range(S)]),
        "ncells.csv": pd.DataFrame({"Number of cells": ncells}, index=[f"s{i}" for i in range(S)]),
        "fractions.csv": pd.DataFrame([rng.dirichlet(np.full(K, 4.0))], index=["Fraction"], columns=names),
        "st_types.csv": pd.DataFrame({"CellType": [names[t] for t in st_type]}, index=[f"s{i}" for i in range(S)]),
    }
    for name in files:
        files[name].index.name = "ID" if name != "fractions.csv" else None
    return files


RUNS = {
    # (enough cells of every type that no cell is drawn twice -- two equal cells are an exact tie of the LAP -- except in the
    #  place-holder run, whose made-up cells are all distinct)
    # Visium-like with a given number of cells per spot
    "visium_ncpsp": (11, {}, dict(n_cells_per_spot_path="ncells.csv", cell_type_fraction_estimation_path="fractions.csv")),
    # cells per spot estimated from the ST counts; place-holder cells for the types that are short
    "estimated_placeholders": (12, dict(C=36), dict(n_cells_per_spot_path=None, cell_type_fraction_estimation_path="fractions.csv",
                                            sampling_method="place_holders")),
    # sub-spot partitions; no downsampling
    "subspots_nodownsample": (13, {}, dict(n_cells_per_spot_path="ncells.csv", cell_type_fraction_estimation_path="fractions.csv",
                                           sampling_sub_spots=True, number_of_selected_sub_spots=17, downsample_off=True)),
    # single-cell ST with its spot cell types: partitions by type
    "single_cell_types": (14, dict(single=True), dict(n_cells_per_spot_path=None, st_cell_type_path="st_types.csv",
                                                      single_cell=True, number_of_selected_spots=7)),
    # single-cell ST from fractions only: shuffled partitions
    "single_cell_fractions": (15, dict(single=True), dict(n_cells_per_spot_path=None, cell_type_fraction_estimation_path="fractions.csv",
                                                          single_cell=True, number_of_selected_spots=9)),
}
COMMON = dict(scRNA_max_transcripts_per_cell=120, number_of_processors=2, seed=3, plot_off=True)


def main():
    gv = {}
    cwd = os.getcwd()
    for tag, (seed, shape, kw) in RUNS.items():
        files = inputs(seed, **shape)
        with tempfile.TemporaryDirectory() as d:
            os.chdir(d)
            try:
                for name, df in files.items():
                    df.to_csv(name)
                    gv[f"{tag}::in::{name}"] = np.frombuffer(open(name, "rb").read(), dtype=np.uint8)
                args = dict(scRNA_path="scRNA.csv", cell_type_path="cell_types.csv", st_path="st.csv", coordinates_path="coords.csv",
                            st_cell_type_path=None, output_folder="out", **COMMON)
                args.update(kw)
                del UNSTABLE[:]
                ref.main_cytospace(**args)
                if UNSTABLE:
                    raise SystemExit(f"{tag}: spot-level answer changes in float32 for LAPs of shape {UNSTABLE}; change the seed")
                gv[f"{tag}::args"] = np.frombuffer(json.dumps(args).encode(), dtype=np.uint8)
                for root, _, fs in os.walk("out"):
                    for f in sorted(fs):
                        rel = os.path.relpath(os.path.join(root, f), "out")
                        gv[f"{tag}::out::{rel}"] = np.frombuffer(open(os.path.join(root, f), "rb").read(), dtype=np.uint8)
            finally:
                os.chdir(cwd)
    np.savez_compressed(OUT, **gv)
    print("gv14:", len(RUNS), "runs,", len(gv), "entries,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
