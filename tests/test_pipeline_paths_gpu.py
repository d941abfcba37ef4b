"""main_cytospace on the paths gv14's five runs never take, against whole runs of the reference's own driver
(tests/golden/gv15_main.npz and gv15_main_large.npz, written by tests/golden/make_golden_main2.py): the other two metrics, 10x
MatrixMarket inputs, tab-separated tables, place-holders in single-cell mode, a cell type short of cells under `duplicates`, a
square result, an output prefix, a LAP of 578 rows and sub-spot chunks of 150.

Every device stage of the driver has a host fallback that gives the same files, so the files alone cannot tell whether a stage
ran.  Each run therefore also wraps the stages (the driver looks their names up when it calls them), has every one report what it
did (`return_info` / `return_words`), and holds the report to the table PATHS: which reader read the two expression inputs and on
which path, what dtype it handed on, whether downsampling and the place-holder generator ran, and what the writer did.

There are no tolerances here: files are equal byte for byte, or -- for the partitioned runs and for `duplicates_short`, whose
repeated cells an exact solver may swap -- as sets of rows without UniqueCID (tests/_pipeline.py); path reports are equal."""
import os
import subprocess
import sys

import pytest

from _pipeline import ROOT, Fixture, _argv, _compare, _folder, _stage

GOLD = Fixture("gv15_main.npz", "gv15_main_large.npz")
CHUNKED = {"single_cell_placeholders", "larger_estimated_subspots", "duplicates_short"}

# run: reader (the stage that reads both expression inputs), the field / dtype it hands on, downsample (is downsample_device
# called), writer ((path, field or refusal) of write_mtx_device; None: not called), place_holders (is place_holders_device called)
_TABLE = dict(reader="read_file_device", field=None, dtype="int64", downsample=True, writer=("device", "integer"), place_holders=False)
PATHS = {
    "spearman": _TABLE,
    "euclidean": _TABLE,
    "tab_separated": _TABLE,
    "duplicates_short": _TABLE,
    "larger": _TABLE,
    "larger_estimated_subspots": _TABLE,
    "square_result": dict(_TABLE, writer=("scipy", "square")),
    "single_cell_placeholders": dict(_TABLE, writer=None, place_holders=True),
    "mtx_integer": dict(_TABLE, reader="read_mtx_device", field="integer"),
    "mtx_real": dict(_TABLE, reader="read_mtx_device", field="real", dtype="float64", downsample=False, writer=("device", "real")),
}
READERS = ("read_file_device", "read_mtx_device")


class Stages:
    """The driver's five device stages wrapped: each call runs the stage itself with its report switched on and keeps the report."""

    def __init__(self, monkeypatch):
        import cytospace_amd.common as common
        import cytospace_amd.post_processing as post
        self.calls = {name: [] for name in READERS + ("downsample_device", "place_holders_device", "write_mtx_device")}

        def reader(name):
            stage = getattr(common, name)

            def wrapped(*a, **k):
                df, info = stage(*a, return_info=True, **k)
                self.calls[name].append(dict(info, dtypes=sorted({str(t) for t in df.dtypes})))
                return df
            monkeypatch.setattr(common, name, wrapped)
        for name in READERS:
            reader(name)
        downsample, place_holders, write = common.downsample_device, common.place_holders_device, post.write_mtx_device

        def downsample_device(data_df, *a, **k):
            df, words = downsample(data_df, *a, return_words=True, **k)
            self.calls["downsample_device"].append({"words": words, "dtypes": sorted({str(t) for t in data_df.dtypes})})
            return df

        def place_holders_device(own, short, *a, **k):
            out, words = place_holders(own, short, *a, return_words=True, **k)
            self.calls["place_holders_device"].append({"short": int(short), "words": words, "shape": out.shape})
            return out

        def write_mtx_device(*a, **k):
            info = write(*a, return_info=True, **k)
            self.calls["write_mtx_device"].append(info)

        monkeypatch.setattr(common, "downsample_device", downsample_device)
        monkeypatch.setattr(common, "place_holders_device", place_holders_device)
        monkeypatch.setattr(post, "write_mtx_device", write_mtx_device)


def _reference_nnz(tag, prefix):
    """The non-zeros of the matrix the reference wrote: the third token of its size line."""
    lines = GOLD.files(tag, "out")[prefix + "assigned_expression/matrix.mtx"].split(b"\n", 3)
    assert lines[0].startswith(b"%%MatrixMarket") and lines[1].startswith(b"%")
    return int(lines[2].split()[2])


def _check_paths(tag, calls, args):
    want = PATHS[tag]
    print(tag, {k: [{f: c[f] for f in c if not f.endswith("_s")} for c in v] for k, v in calls.items()})
    other = READERS[1 - READERS.index(want["reader"])]
    reads = calls[want["reader"]]
    assert len(reads) == 2 and calls[other] == [], (tag, calls)
    for r in reads:                                        # ST first, then scRNA
        assert r["path"] == "device", (tag, r)
        assert r["dtypes"] == [want["dtype"]], (tag, r)
        if want["field"] is not None:
            assert r["field"] == want["field"], (tag, r)
    assert want["downsample"] == (not args.get("downsample_off", False))
    assert len(calls["downsample_device"]) == (1 if want["downsample"] else 0), (tag, calls["downsample_device"])
    for d in calls["downsample_device"]:
        assert d["dtypes"] == [want["dtype"]] and d["words"] > 0, (tag, d)      # (every run's cells exceed the target: draws)
    if want["place_holders"]:
        assert len(calls["place_holders_device"]) >= 1 and all(c["short"] > 0 and c["shape"][1] == c["short"]
                                                                  for c in calls["place_holders_device"]), (tag, calls)
    else:
        assert calls["place_holders_device"] == [], (tag, calls)
    writes = calls["write_mtx_device"]
    if want["writer"] is None:
        assert writes == [], (tag, writes)
        return
    assert len(writes) == 1, (tag, writes)
    w = writes[0]
    if want["writer"][0] == "device":
        assert (w["path"], w["field"]) == want["writer"], (tag, w)
        assert w["nnz"] == _reference_nnz(tag, args.get("output_prefix", "")), (tag, w)
    else:
        assert (w["path"], w["reason"]) == want["writer"], (tag, w)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(PATHS))
def test_run_equals_the_reference_and_takes_its_device_paths(tag, tmp_path, monkeypatch):
    from cytospace_amd.cytospace import main_cytospace
    args = _stage(GOLD, tag, tmp_path)
    monkeypatch.chdir(tmp_path)
    stages = Stages(monkeypatch)
    main_cytospace(**args)
    _compare(GOLD, tag, tmp_path / args["output_folder"], tag in CHUNKED, args.get("output_prefix", ""))
    _check_paths(tag, stages.calls, args)


# two logical ranks on one GPU.  `spearman` and `larger` are one LAP each (one device solves it; the list only has to be taken);
# the sub-spot run spreads its chunks over both ranks, and the in-process communicator broadcasts the ST operand of its metric.
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["spearman", "larger", "larger_estimated_subspots"])
def test_two_logical_devices_equal_the_reference_run(tag, tmp_path, monkeypatch):
    from cytospace_amd.cytospace import main_cytospace
    args = _stage(GOLD, tag, tmp_path)
    monkeypatch.chdir(tmp_path)
    main_cytospace(devices=[0, 0], **args)
    _compare(GOLD, tag, tmp_path / args["output_folder"], tag in CHUNKED, args.get("output_prefix", ""))


@pytest.mark.gpu
@pytest.mark.parametrize("tag, flags", [("euclidean", ("-dm",)), ("larger_estimated_subspots", ("-op", "-sss", "-nosss")),
                                        ("single_cell_placeholders", ("-sam", "-sc", "-noss"))])
def test_command_line_equals_the_reference_run(tag, flags, tmp_path):
    args = _stage(GOLD, tag, tmp_path)
    argv = [sys.executable, "-m", "cytospace_amd"] + _argv(args)
    assert set(flags) <= set(argv), argv
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(argv, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _compare(GOLD, tag, tmp_path / args["output_folder"], tag in CHUNKED, args.get("output_prefix", ""))


@pytest.mark.gpu
def test_two_calls_in_one_process_write_the_same_folder(tmp_path, monkeypatch):
    """`larger` twice: every file byte for byte, the log too but for the lines that hold a clock reading."""
    from cytospace_amd.cytospace import main_cytospace
    folders = []
    for k in ("first", "second"):
        d = tmp_path / k
        d.mkdir()
        args = _stage(GOLD, "larger", d)
        monkeypatch.chdir(d)
        main_cytospace(**args)
        folders.append(_folder(d / args["output_folder"]))
    clock = ("Start time", "Time to ", "Total execution time")
    for f in folders:
        f["log.txt"] = b"\n".join(ln for ln in f["log.txt"].split(b"\n") if not ln.decode().startswith(clock))
    assert sorted(folders[0]) == sorted(folders[1]) and len(folders[0]) == 7
    for name in folders[0]:
        assert folders[0][name] == folders[1][name], name
    assert b"distance_metric: Pearson_correlation" in folders[0]["log.txt"]
