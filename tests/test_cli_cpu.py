"""CPU tests of the command line (cytospace_amd/argument_parser.py, python -m cytospace_amd) and of the driver's refusals:
the reference's flags (cytospace/common/argument_parser.py) with their short forms, defaults and choices, written out here
as a literal table; the solver choices are this package's, with lapjv_hip the default."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# dest: (short, long, default, choices, required, kind)
REFERENCE = {
    "scRNA_path": ("-sp", "--scRNA-path", None, None, True, str),
    "cell_type_path": ("-ctp", "--cell-type-path", None, None, True, str),
    "st_path": ("-stp", "--st-path", None, None, False, str),
    "coordinates_path": ("-cp", "--coordinates-path", None, None, False, str),
    "spaceranger_path": ("-srp", "--spaceranger-path", None, None, False, str),
    "st_cell_type_path": ("-stctp", "--st-cell-type-path", None, None, False, str),
    "cell_type_fraction_estimation_path": ("-ctfep", "--cell-type-fraction-estimation-path", None, None, False, str),
    "n_cells_per_spot_path": ("-ncpsp", "--n-cells-per-spot-path", None, None, False, str),
    "output_folder": ("-o", "--output-folder", "cytospace_results", None, False, str),
    "output_prefix": ("-op", "--output-prefix", "", None, False, str),
    "mean_cell_numbers": ("-mcn", "--mean-cell-numbers", 5, None, False, int),
    "downsample_off": (None, "--downsample-off", False, None, False, "flag"),
    "scRNA_max_transcripts_per_cell": ("-smtpc", "--scRNA_max_transcripts_per_cell", 1500, None, False, int),
    "single_cell": ("-sc", "--single-cell", False, None, False, "flag"),
    "number_of_selected_spots": ("-noss", "--number-of-selected-spots", 10000, None, False, int),
    "sampling_sub_spots": ("-sss", "--sampling-sub-spots", False, None, False, "flag"),
    "number_of_selected_sub_spots": ("-nosss", "--number-of-selected-sub-spots", 10000, None, False, int),
    "number_of_processors": ("-nop", "--number-of-processors", 4, None, False, int),
    "solver_method": ("-sm", "--solver-method", "lapjv_hip", ["lapjv", "lapjv_compat", "lap_CSPR", "lapjv_hip"], False, None),
    "distance_metric": ("-dm", "--distance-metric", "Pearson_correlation",
                        ["Pearson_correlation", "Spearman_correlation", "Euclidean"], False, None),
    "sampling_method": ("-sam", "--sampling-method", "duplicates", ["duplicates", "place_holders"], False, None),
    "seed": ("-se", "--seed", 1, None, False, int),
    "plot_off": ("-p", "--plot-off", False, None, False, "flag"),
    "geometry": ("-g", "--geometry", "honeycomb", None, False, str),
    "num_column": ("-nc", "--num-column", 3, None, False, int),
    "max_num_cells_plot": ("-mp", "--max-num-cells-plot", 50000, None, False, int),
}


def test_parser_matches_the_reference_table():
    import argparse
    from cytospace_amd.argument_parser import build_parser
    actions = {a.dest: a for a in build_parser()._actions if a.dest != "help"}
    assert sorted(actions) == sorted(REFERENCE)
    for dest, (short, long_, default, choices, required, kind) in REFERENCE.items():
        a = actions[dest]
        assert a.option_strings == ([short] if short else []) + [long_], dest
        assert a.default == default, dest
        assert (list(a.choices) if a.choices is not None else None) == choices, dest
        assert a.required == required, dest
        if kind == "flag":
            assert isinstance(a, argparse._StoreTrueAction), dest
        elif kind is not None:
            assert a.type is kind, dest


def test_parse_gives_main_cytospace_keywords():
    import inspect
    from cytospace_amd.argument_parser import argument_parser
    from cytospace_amd.cytospace import main_cytospace
    args = argument_parser(["-sp", "a.csv", "-ctp", "b.csv", "-stp", "c.csv", "-cp", "d.csv", "-ctfep", "e.csv", "-sc", "-nop", "2"])
    assert args["scRNA_path"] == "a.csv" and args["single_cell"] is True and args["number_of_processors"] == 2
    params = inspect.signature(main_cytospace).parameters
    assert set(args) <= set(params)
    assert params["solver_method"].default == "lapjv_hip" and "devices" in params


def test_help_exits_zero_in_a_fresh_process():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "cytospace_amd", "--help"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--scRNA-path" in r.stdout and "--solver-method" in r.stdout


@pytest.fixture
def no_device(monkeypatch):
    from cytospace_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "device_count", refuse)


BASE = dict(scRNA_path="sc.csv", cell_type_path="ct.csv", n_cells_per_spot_path=None, st_cell_type_path=None,
            cell_type_fraction_estimation_path="frac.csv", st_path="st.csv", coordinates_path="xy.csv", output_folder="out")


@pytest.mark.parametrize("change,needle", [(dict(spaceranger_path="x.tar.gz", st_path=None, coordinates_path=None), "scanpy"),
                                           (dict(cell_type_fraction_estimation_path=None), "R"),
                                           (dict(solver_method="lapjv"), "lapjv_hip"),
                                           (dict(solver_method="lap_CSPR"), "lapjv_hip")])
def test_unsupported_paths_fail_before_any_device_work(change, needle, tmp_path, monkeypatch, no_device):
    from cytospace_amd.cytospace import main_cytospace
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=needle):
        main_cytospace(**dict(BASE, **change))
    assert not (tmp_path / "out").exists()


def test_unsupported_paths_on_the_command_line(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "cytospace_amd", "-sp", "a", "-ctp", "b", "-stp", "c", "-cp", "d"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ValueError" in r.stderr and "-ctfep" in r.stderr


def test_check_paths(tmp_path, monkeypatch, capsys):
    from cytospace_amd.common import check_paths
    monkeypatch.chdir(tmp_path)
    p = check_paths("a/b", "x_")
    assert p == os.path.join(str(tmp_path), "a/b") and os.path.isdir(p)
    open(os.path.join(p, "x_assigned_locations.csv"), "w").close()
    check_paths("a/b", "x_")
    assert "overwrite" in capsys.readouterr().out
