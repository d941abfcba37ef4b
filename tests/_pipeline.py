"""What the whole-run tests share (test_pipeline_gpu.py on gv14, test_pipeline_paths_gpu.py on gv15): a fixture of reference runs
in the key layout `tag::args`, `tag::in::<relative path>`, `tag::out::<relative path>` (tests/golden/make_golden_main.py), staging
a run's input files and comparing an output folder with the reference's.  The reference concatenates the chunks of a partitioned
run in completion order, so such runs are compared row-set-wise; the others byte for byte."""
import io
import json
import os

import numpy as np
import pandas as pd
import scipy.io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_ARGS = ("scRNA_path", "cell_type_path", "st_path", "coordinates_path", "n_cells_per_spot_path",
            "cell_type_fraction_estimation_path", "st_cell_type_path", "output_folder", "mean_cell_numbers", "downsample_off",
            "scRNA_max_transcripts_per_cell", "plot_off", "geometry", "output_prefix", "seed", "sampling_method",
            "distance_metric", "single_cell", "sampling_sub_spots")
FLAGS = {"scRNA_path": "-sp", "cell_type_path": "-ctp", "st_path": "-stp", "coordinates_path": "-cp",
         "n_cells_per_spot_path": "-ncpsp", "cell_type_fraction_estimation_path": "-ctfep", "st_cell_type_path": "-stctp",
         "output_folder": "-o", "scRNA_max_transcripts_per_cell": "-smtpc", "number_of_processors": "-nop", "seed": "-se",
         "sampling_method": "-sam", "number_of_selected_sub_spots": "-nosss", "number_of_selected_spots": "-noss",
         "solver_method": "-sm", "distance_metric": "-dm", "output_prefix": "-op"}
SWITCHES = {"downsample_off": "--downsample-off", "single_cell": "-sc", "sampling_sub_spots": "-sss", "plot_off": "-p"}


class Fixture:
    """The entries of one or more .npz files under tests/golden, read once."""

    def __init__(self, *names):
        self.paths = [os.path.join(ROOT, "tests", "golden", n) for n in names]
        self.entries = {}
        for p in self.paths:
            with np.load(p) as z:
                self.entries.update({k: z[k].tobytes() for k in z.files})
        self.runs = sorted({k.split("::")[0] for k in self.entries})

    def args(self, tag):
        return json.loads(self.entries[f"{tag}::args"].decode())

    def files(self, tag, kind):
        """{relative path: bytes} of a run's "in" or "out" files."""
        lead = f"{tag}::{kind}::"
        return {k[len(lead):]: v for k, v in self.entries.items() if k.startswith(lead)}


def _stage(gold, tag, d):
    for rel, data in gold.files(tag, "in").items():
        (d / rel).parent.mkdir(parents=True, exist_ok=True)
        (d / rel).write_bytes(data)
    args = gold.args(tag)
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


def _folder(out_dir):
    got = {}
    for root, _, fs in os.walk(out_dir):
        for f in fs:
            got[os.path.relpath(os.path.join(root, f), out_dir)] = open(os.path.join(root, f), "rb").read()
    return got


def _compare(gold, tag, out_dir, chunked, prefix=""):
    """The files under out_dir against the reference's of run `tag`; chunked: row-set-wise (UniqueCID dropped, rows sorted, matrix
    columns sorted) instead of byte for byte.  prefix: the run's output_prefix."""
    want = gold.files(tag, "out")
    got = _folder(out_dir)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name, ref in want.items():
        mine = got[name]
        assert name.startswith(prefix), name
        if name == prefix + "log.txt":
            lines = lambda b: {ln.split(": ")[0]: ln for ln in b.decode().splitlines() if ": " in ln}   # noqa: E731
            a, b = lines(mine), lines(ref)
            for key in LOG_ARGS + ("Number of genes used for mapping", "Number of spots satisfying input for mapping",
                                   "Number of cells satisfying input for mapping"):
                assert a[key] == b[key], key
            assert a["solver_method"] == "solver_method: lapjv_hip"
        elif name == prefix + "assigned_locations.csv":
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


def _argv(args):
    """main_cytospace's keyword arguments as the flags of `python -m cytospace_amd`."""
    argv = []
    for k, v in args.items():
        if k in SWITCHES:
            argv += [SWITCHES[k]] if v else []
        elif v is not None:
            argv += [FLAGS[k], str(v)]
    return argv
