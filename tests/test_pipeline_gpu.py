"""main_cytospace and `python -m cytospace_amd` end to end on the GPU, against whole runs of the reference's own driver
(tests/golden/gv14_main.npz, written by tests/golden/make_golden_main.py): same inputs, same arguments (solver lapjv_hip),
same output files.  The reference concatenates the chunks of a partitioned run in completion order, so those runs are
compared row-set-wise; the unpartitioned runs byte for byte."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import scipy.io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "gv14_main.npz"))
RUNS = sorted({k.split("::")[0] for k in GOLD.files})
CHUNKED = {"subspots_nodownsample", "single_cell_types", "single_cell_fractions"}
LOG_ARGS = ("scRNA_path", "cell_type_path", "st_path", "coordinates_path", "n_cells_per_spot_path",
            "cell_type_fraction_estimation_path", "st_cell_type_path", "output_folder", "mean_cell_numbers", "downsample_off",
            "scRNA_max_transcripts_per_cell", "plot_off", "geometry", "output_prefix", "seed", "sampling_method",
            "distance_metric", "single_cell", "sampling_sub_spots")


def _stage(tag, d):
    for k in GOLD.files:
        if k.startswith(f"{tag}::in::"):
            (d / k.split("::")[2]).write_bytes(GOLD[k].tobytes())
    args = json.loads(GOLD[f"{tag}::args"].tobytes().decode())
    args["solver_method"] = "lapjv_hip"
    return args


def _rows(text, drop_first=False):
    df = pd.read_csv(io.StringIO(text))
    if drop_first:
        df = df.iloc[:, 1:]
    return sorted(map(tuple, df.astype(str).to_numpy().tolist())), list(df.columns)


def _mtx_columns(data):
    m = scipy.io.mmread(io.BytesIO(data)).toarray()
    return sorted(map(tuple, m.T.tolist()))


def _compare(tag, out_dir):
    want = {k.split("::")[2]: GOLD[k].tobytes() for k in GOLD.files if k.startswith(f"{tag}::out::")}
    got = {}
    for root, _, fs in os.walk(out_dir):
        for f in fs:
            got[os.path.relpath(os.path.join(root, f), out_dir)] = open(os.path.join(root, f), "rb").read()
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    chunked = tag in CHUNKED
    for name, ref in want.items():
        mine = got[name]
        if name == "log.txt":
            lines = lambda b: {ln.split(": ")[0]: ln for ln in b.decode().splitlines() if ": " in ln}   # noqa: E731
            a, b = lines(mine), lines(ref)
            for key in LOG_ARGS + ("Number of genes used for mapping", "Number of spots satisfying input for mapping",
                                   "Number of cells satisfying input for mapping"):
                assert a[key] == b[key], key
            assert a["solver_method"] == "solver_method: lapjv_hip"
        elif name == "assigned_locations.csv":
            if chunked:                      # UniqueCID numbers follow the chunk order: compare the rest of every row
                assert _rows(mine.decode(), True) == _rows(ref.decode(), True), name
            else:
                assert mine == ref, name
        elif name.endswith("matrix.mtx") and chunked:
            assert _mtx_columns(mine) == _mtx_columns(ref), name
        elif name.endswith(".csv") and chunked:
            assert _rows(mine.decode()) == _rows(ref.decode()), name
        else:
            assert mine == ref, name


@pytest.mark.gpu
@pytest.mark.parametrize("tag", RUNS)
def test_main_cytospace_equals_the_reference_run(tag, tmp_path, monkeypatch):
    from cytospace_amd.cytospace import main_cytospace
    args = _stage(tag, tmp_path)
    monkeypatch.chdir(tmp_path)
    main_cytospace(**args)
    _compare(tag, tmp_path / args["output_folder"])


FLAGS = {"scRNA_path": "-sp", "cell_type_path": "-ctp", "st_path": "-stp", "coordinates_path": "-cp",
         "n_cells_per_spot_path": "-ncpsp", "cell_type_fraction_estimation_path": "-ctfep", "st_cell_type_path": "-stctp",
         "output_folder": "-o", "scRNA_max_transcripts_per_cell": "-smtpc", "number_of_processors": "-nop", "seed": "-se",
         "sampling_method": "-sam", "number_of_selected_sub_spots": "-nosss", "number_of_selected_spots": "-noss",
         "solver_method": "-sm"}
SWITCHES = {"downsample_off": "--downsample-off", "single_cell": "-sc", "sampling_sub_spots": "-sss", "plot_off": "-p"}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["visium_ncpsp", "single_cell_types"])
def test_command_line_equals_the_reference_run(tag, tmp_path):
    args = _stage(tag, tmp_path)
    argv = [sys.executable, "-m", "cytospace_amd"]
    for k, v in args.items():
        if k in SWITCHES:
            argv += [SWITCHES[k]] if v else []
        elif v is not None:
            argv += [FLAGS[k], str(v)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(argv, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _compare(tag, tmp_path / args["output_folder"])
