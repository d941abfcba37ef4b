"""main_cytospace(resident=True) on every whole run of the fixtures (gv14_main.npz, gv15_main.npz, gv15_main_large.npz): the
files equal the reference's under the rule of the existing whole-run tests (tests/_pipeline.py: byte for byte, or row-set-wise
for the partitioned runs), they equal the files of a resident=False run of the same arguments in the same test byte for byte
(log.txt but for its clock readings), and resident.last_run -- which table stayed on the device, how often its values were
fetched, which stage went through the host -- is held to the literal table RUNS.

Both runs get devices=[0]: a matrix stays resident only when one device solves every chunk, whatever the machine has."""
import copy

import pytest

from _pipeline import Fixture, _compare, _folder, _stage

GOLD14, GOLD15 = Fixture("gv14_main.npz"), Fixture("gv15_main.npz", "gv15_main_large.npz")
CHUNKED = {"subspots_nodownsample", "single_cell_types", "single_cell_fractions",
           "single_cell_placeholders", "larger_estimated_subspots", "duplicates_short"}

# run: (source of both tables, fetches of the scRNA values, fetches of the ST values, fallbacks).  The ST values are fetched once
# where the cells per spot are estimated from them (no n_cells_per_spot file, not single-cell); the scRNA values where the
# place-holder sampler builds its cells on the host and where the writer's refusal hands the matrix to scipy.
_T = ("table", 0, 0, [])
RUNS = {
    "visium_ncpsp": _T,
    "subspots_nodownsample": _T,
    "single_cell_fractions": _T,
    "single_cell_types": _T,
    "estimated_placeholders": ("table", 1, 1, [("sample", "place_holders")]),
    "duplicates_short": _T,
    "euclidean": _T,
    "spearman": _T,
    "tab_separated": _T,
    "larger": _T,
    "larger_estimated_subspots": ("table", 0, 1, []),
    "square_result": ("table", 1, 0, [("write_mtx", "square")]),
    "single_cell_placeholders": ("table", 1, 0, [("sample", "place_holders")]),
    "mtx_integer": ("upload", 0, 0, []),
    "mtx_real": ("upload", 0, 0, []),
}
CLOCK = ("Start time", "Time to ", "Total execution time")


def test_the_table_names_every_run():
    assert sorted(RUNS) == sorted(GOLD14.runs + GOLD15.runs)


def _without_clock(files, prefix):
    files = dict(files)
    name = prefix + "log.txt"
    files[name] = b"\n".join(ln for ln in files[name].split(b"\n") if not ln.decode().startswith(CLOCK))
    return files


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(RUNS))
def test_resident_run_equals_the_reference_and_the_host_run(tag, tmp_path, monkeypatch):
    from cytospace_amd import resident
    from cytospace_amd.cytospace import main_cytospace
    gold = GOLD14 if tag in GOLD14.runs else GOLD15
    folders = {}
    for leg in ("host", "resident"):
        d = tmp_path / leg
        d.mkdir()
        args = _stage(gold, tag, d)
        monkeypatch.chdir(d)
        resident.last_run = {"stale": True}
        main_cytospace(**args, devices=[0], resident=(leg == "resident"))
        if leg == "host":
            assert resident.last_run == {"stale": True}          # (the switch off: nothing of the resident path runs)
        else:
            report = copy.deepcopy(resident.last_run)
        prefix = args.get("output_prefix", "")
        _compare(gold, tag, d / args["output_folder"], tag in CHUNKED, prefix)
        folders[leg] = _without_clock(_folder(d / args["output_folder"]), prefix)
    assert sorted(folders["host"]) == sorted(folders["resident"])
    for name in folders["host"]:
        assert folders["resident"][name] == folders["host"][name], name
    print(tag, report)
    source, sc_fetches, st_fetches, fallbacks = RUNS[tag]
    assert sorted(report) == ["ST", "fallbacks", "scRNA"]
    assert report["scRNA"]["source"] == source and report["ST"]["source"] == source
    assert report["scRNA"]["fetches"] == sc_fetches and report["ST"]["fetches"] == st_fetches
    assert report["fallbacks"] == fallbacks
    assert report["scRNA"]["materialized"] >= 1 and report["ST"]["materialized"] >= 1      # (each reached a stage on the device)


@pytest.mark.gpu
def test_the_environment_variable_is_the_switch(tmp_path, monkeypatch):
    from cytospace_amd import resident
    from cytospace_amd.cytospace import main_cytospace
    args = _stage(GOLD14, "visium_ncpsp", tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("CYTOSPACE_HIP_RESIDENT", "1")
    resident.last_run = {}
    main_cytospace(**args, devices=[0])
    assert resident.last_run["scRNA"]["source"] == "table" and resident.last_run["scRNA"]["fetches"] == 0
    _compare(GOLD14, "visium_ncpsp", tmp_path / args["output_folder"], False)
    monkeypatch.setenv("CYTOSPACE_HIP_RESIDENT", "0")
    resident.last_run = {}
    main_cytospace(**dict(args, output_prefix="again_"), devices=[0])
    assert resident.last_run == {}
