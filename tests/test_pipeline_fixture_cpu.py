"""The gv15 fixture itself (tests/golden/make_golden_main2.py), without a GPU: every run is complete, the runs are the ones the
GPU test's path table names, and the runs built to reach one particular path do hold what takes the driver there."""
import io
import os

import pandas as pd
import scipy.io

import test_pipeline_paths_gpu as T

GOLD = T.GOLD
CAP = 621726                       # tests/golden/gv5_solve_lap.npz, the largest fixture committed before gv15
PATH_ARGS = ("scRNA_path", "cell_type_path", "st_path", "coordinates_path", "n_cells_per_spot_path",
             "cell_type_fraction_estimation_path", "st_cell_type_path")


def test_every_run_has_its_arguments_inputs_and_assignments():
    assert len(GOLD.runs) == 10
    for tag in GOLD.runs:
        args = GOLD.args(tag)
        named = [args[k] for k in PATH_ARGS if args.get(k) is not None]
        assert len(named) >= 4, (tag, named)
        inputs = GOLD.files(tag, "in")
        assert set(named) <= set(inputs), (tag, named, sorted(inputs))
        assert args.get("output_prefix", "") + "assigned_locations.csv" in GOLD.files(tag, "out"), tag
        assert "solver_method" not in args                   # (the reference's default; the tests set lapjv_hip)


def test_the_runs_are_the_path_tables():
    assert set(GOLD.runs) == set(T.PATHS)
    assert T.CHUNKED <= set(T.PATHS)


def test_square_result_is_square():
    m = scipy.io.mmread(io.BytesIO(GOLD.files("square_result", "out")["assigned_expression/matrix.mtx"]))
    assert m.shape[0] == m.shape[1] == 88


def test_duplicates_short_assigns_cells_twice():
    ids = pd.read_csv(io.BytesIO(GOLD.files("duplicates_short", "out")["assigned_locations.csv"])).OriginalCID
    assert ids.duplicated().any() and ids.nunique() < len(ids)


def test_single_cell_placeholders_has_generated_cells():
    made = pd.read_csv(io.BytesIO(GOLD.files("single_cell_placeholders", "out")["new_scRNA.csv"]), index_col=0)
    assert made.shape[1] > 0
    assert sorted(GOLD.files("single_cell_placeholders", "out")) == ["assigned_locations.csv", "log.txt", "new_scRNA.csv"]


def test_matrix_market_inputs_have_the_banners_of_their_runs():
    for tag, field in (("mtx_real", b"real"), ("mtx_integer", b"integer")):
        args, inputs = GOLD.args(tag), GOLD.files(tag, "in")
        lists = set()
        for key in ("scRNA_path", "st_path"):
            path = args[key]
            assert path.endswith("/matrix.mtx")
            assert inputs[path].split(b"\n", 1)[0] == b"%%MatrixMarket matrix coordinate " + field + b" general", (tag, key)
            lists |= {os.path.basename(p) for p in inputs if p.startswith(os.path.dirname(path) + "/")} - {"matrix.mtx"}
        assert lists == {"genes.tsv", "barcodes.tsv", "features.tsv", "cells.csv"}, (tag, lists)
    st = scipy.io.mmread(io.BytesIO(GOLD.files("mtx_real", "in")[GOLD.args("mtx_real")["st_path"]])).toarray()
    sc = scipy.io.mmread(io.BytesIO(GOLD.files("mtx_real", "in")[GOLD.args("mtx_real")["scRNA_path"]])).toarray()
    assert (st != st.round()).any() and (st * 4 == (st * 4).round()).all()          # quarters
    assert (sc == sc.round()).all()                                                  # whole numbers in a `real` file


def test_tab_separated_inputs_are():
    args, inputs = GOLD.args("tab_separated"), GOLD.files("tab_separated", "in")
    assert (args["scRNA_path"], args["st_path"]) == ("scRNA.tsv", "st.txt")
    for key in ("scRNA_path", "st_path"):
        head = inputs[args[key]].split(b"\n", 1)[0]
        assert head.count(b"\t") > 0 and b"," not in head


def test_no_fixture_file_is_larger_than_the_largest_before_it():
    for path in GOLD.paths:
        assert os.path.getsize(path) <= CAP, path
