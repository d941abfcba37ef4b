"""cyto_table_read / cyto_table_fetch (csrc/table.hip) against the plain model of oracle/table.py on the files of
tools/table_cases.py: every file aimed at one boundary of the kernels (64 KiB blocks and 256-byte thread spans of tbl_lines,
16-byte slices and 4 KiB rounds of tbl_fields, 16 MiB upload chunks, the block scan's carry), the refusals with the line and
byte they name, and which of two defects is reported.  Both sides are integer words: the comparison is exact.  The model itself is
held to pandas on the same files by tests/test_read_table_model_cpu.py.

Then the converter as compiled for the device on 10^6 tokens, a file above 2^32 bytes, and repeated and concurrent calls."""
import collections
import os
import shutil
import threading
import time

import numpy as np
import pandas as pd
import pytest

from oracle.table import KIND_NAMES, QUOTE, parse_spans, read_device, table_model
from tools import table_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.cases()
FAMILIES = sorted({c.family for c in CASES})
THROUGH_READER = 4 << 20            # files up to this size also go through read_file_device, against read_file


def _equal(a, b):
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    for c in range(a.shape[1]):
        x, y = a.iloc[:, c].to_numpy(), b.iloc[:, c].to_numpy()
        assert x.dtype == y.dtype
        if x.dtype == np.float64:
            assert np.array_equal(x.view(np.int64), y.view(np.int64))


def _same(got, want, name):
    assert got["status"] == want["status"], (name, got.get("reason"), want.get("reason"))
    if want["status"]:
        assert tuple(got["reason"]) == tuple(want["reason"]), name
        return
    assert (got["G"], got["C"]) == (want["G"], want["C"]), name
    assert np.array_equal(got["is_float"], want["is_float"]), name
    bad = np.argwhere(got["values"] != want["values"])
    assert bad.size == 0, (name, len(bad), [(tuple(i), int(got["values"][tuple(i)]), int(want["values"][tuple(i)])) for i in bad[:5]])
    assert got["labels"].tobytes() == want["labels"].tobytes(), name


def _write(path, data):
    if isinstance(data, bytes):
        path.write_bytes(data)
    else:
        data.tofile(path)


def _through_reader(case, data, path, C, d0):
    """read_file_device against read_file, as tests/test_read_table_gpu.py's _device and _fallback do, with the whole reason."""
    from cytospace_amd import common
    first = data[d0:].split(b"\n", 1)[0]
    if d0 >= len(data) or first.count(case.sep) != C:
        return False                # (the reader takes ncols from the first data line: this case is for the direct call only)
    if case.intended == "device":
        got, info = common.read_file_device(str(path), return_info=True)
        if info["path"] == "pandas":
            assert info["reason"]["kind"] == "row labels", (case.name, info)
        _equal(got, common.read_file(str(path)))
        return True
    info = {}
    assert common._table_on_device(str(path), 0, info) is None
    kind, line, byte = case.intended
    if common._table_head(data[:d0], first + b"\n", case.sep.decode(), C) is None:
        # (a defect in the first data line that pandas' parse of the header with that line already stumbles over)
        assert info["reason"]["kind"] == "header", (case.name, info["reason"])
    else:
        assert info["reason"] == {"kind": KIND_NAMES[kind], "line": line, "byte": byte}, (case.name, info["reason"], case.intended)
    try:
        want = common.read_file(str(path))
    except Exception as e:
        with pytest.raises(type(e)):
            common.read_file_device(str(path))
        return True
    got, info = common.read_file_device(str(path), return_info=True)
    assert info["path"] == "pandas"
    _equal(got, want)
    return True


@pytest.mark.parametrize("family", FAMILIES)
def test_device_equals_model(tmp_path, family):
    t = time.perf_counter()
    n = reader = 0
    failed = []                                         # every file is read once: a regression shows its whole pattern in one run
    for case in CASES:
        if case.family != family:
            continue
        data = case.make()
        path = tmp_path / (case.name + (".csv" if case.sep == b"," else ".tsv"))
        _write(path, data)
        d0, C = tc.header_end(data), tc.ncols_of(case, data)
        want = table_model(data, case.sep, d0, C)
        assert ("device" if want["status"] == 0 else want["reason"]) == case.intended, (case.name, want.get("reason"))
        try:
            _same(read_device(path, case.sep, d0, C), want, case.name)
            if len(data) <= THROUGH_READER:
                reader += _through_reader(case, data, path, C, d0)
        except AssertionError as e:
            failed.append((case.name, repr(e)[:300]))
        path.unlink()
        n += 1
    print(f"{family}: {n} files, {reader} of them also through read_file_device, {len(failed)} failed, {time.perf_counter() - t:.1f} s")
    assert n == sum(c.family == family for c in CASES) and n > 0
    assert not failed, (len(failed), failed[:20])


def test_device_converter_on_a_million_tokens(tmp_path):
    """The device compilation of parse_token (its own table of powers, the device's float64 division, subnormal results) against
    the host compilation, which tests/test_read_table_cpu.py holds to pandas: every value word, bit for bit."""
    data, C = tc.million_table()
    path = tmp_path / "million.tsv"
    path.write_bytes(data)
    d0 = tc.header_end(data)
    want = table_model(data, b"\t", d0, C, stats=True)
    assert want["status"] == 0 and want["G"] * want["C"] >= 1_000_000
    print(f"{want['G']} x {want['C']} tokens, {int(want['is_float'].sum())} float64 columns; "
          f"two-step divisions {want['two_step']}, subnormal results {want['subnormal']}")
    assert want["two_step"] >= 1000 and want["subnormal"] >= 1000
    _same(read_device(path, b"\t", d0, C), want, "million tokens")


LINE, HEAD, LEAD = 4096, b"IDX\tvalue\n", 9


def _huge_file(path, G):
    """G lines of LINE bytes, "r<7 digits>\\t<9 digits>.<zeros>\\n"; the last one without its '\\n'.  With a header of 10 bytes the
    token of some line lies over every multiple of 4096: over byte 2^31 and byte 2^32."""
    with open(path, "wb") as f:
        f.write(HEAD)
        for lo in range(0, G, 4096):
            g = np.arange(lo, min(G, lo + 4096))
            a = np.full((len(g), LINE), ord("0"), np.uint8)
            a[:, 0] = ord("r")
            for k in range(7):
                a[:, 7 - k] = 48 + (g // 10**k) % 10
            a[:, 8] = 9
            lead = (g * 7919 + 1) % 10**LEAD
            for k in range(LEAD):
                a[:, 8 + LEAD - k] = 48 + (lead // 10**k) % 10
            a[:, 9 + LEAD] = ord(".")
            a[:, LINE - 1] = 10
            raw = a.tobytes()
            f.write(raw[:-1] if g[-1] == G - 1 else raw)


def test_file_above_4_GiB(tmp_path):
    """Positions beyond 2^31 and 2^32: values from the host converter on the same bytes, labels from construction."""
    G = 1_100_000
    size = len(HEAD) + G * LINE - 1
    free = shutil.disk_usage(tmp_path).free
    if free < 6 * 10**9:
        pytest.skip(f"{free / 1e9:.1f} GB free under {tmp_path}: the {size / 1e9:.1f} GB file needs 6 GB")
    path = tmp_path / "huge.tsv"
    t = time.perf_counter()
    _huge_file(path, G)
    assert os.path.getsize(path) == size and size > 2**32 + 2**27
    buf = np.memmap(path, np.uint8, "r")
    starts = len(HEAD) + np.arange(G, dtype=np.int64) * LINE + 9
    stops = starts + LINE - 10
    for edge in (2**31, 2**32):                         # a token lies over each
        i = int(np.searchsorted(starts, edge)) - 1
        assert starts[i] < edge < stops[i] and buf[edge] == ord("0")
    assert buf[size - 1] == ord("0") and stops[-1] == size
    kind, value, _ = parse_spans(buf, starts, stops)
    assert (kind == 1).all() and len(np.unique(value)) > G // 2
    labels = np.empty((G, 10), np.uint8)
    labels[:, 0] = ord("r")
    for k in range(7):
        labels[:, 7 - k] = 48 + (np.arange(G) // 10**k) % 10
    labels[:, 8], labels[:, 9] = 9, 10
    want = {"status": 0, "G": G, "C": 1, "values": value.view(np.int64).reshape(G, 1), "is_float": np.ones(1, np.int8), "labels": labels.ravel()}
    del buf
    t1 = time.perf_counter()
    _same(read_device(path, b"\t", len(HEAD), 1), want, "huge")
    t2 = time.perf_counter()
    # one refusal beyond 2^32: a '"' inside a token
    q = 2**32 + 123_457
    with open(path, "r+b") as f:
        f.seek(q)
        f.write(b'"')
    got = read_device(path, b"\t", len(HEAD), 1)
    assert got["status"] == 7 and tuple(got["reason"]) == (QUOTE, 2 + (q - len(HEAD)) // LINE, q), got
    print(f"{size / 1e9:.2f} GB: written and expected values in {t1 - t:.1f} s, device read {t2 - t1:.1f} s, refusal {time.perf_counter() - t2:.1f} s")


def test_repeated_and_concurrent_calls(tmp_path):
    """A call takes its own stream and its own error and count words: the same file twice, and two files from two threads at once,
    give the model's words every time."""
    by_name = {c.name: c for c in CASES}
    jobs = []
    for name in ("tall_300001_by_1", "label_over_128k", f"quote_{tc.BLOCK}"):
        case = by_name[name]
        data = case.make()
        path = tmp_path / (name + ".tsv")
        path.write_bytes(data)
        d0, C = tc.header_end(data), tc.ncols_of(case, data)
        jobs.append((name, path, case.sep, d0, C, table_model(data, case.sep, d0, C)))
    for name, path, sep, d0, C, want in jobs:
        for _ in range(2):
            _same(read_device(path, sep, d0, C), want, name)
    failures = []

    def work(job):
        name, path, sep, d0, C, want = job
        try:
            for _ in range(4):
                _same(read_device(path, sep, d0, C), want, name)
        except BaseException as e:                      # noqa: B902 (reported by the test below)
            failures.append((name, repr(e)))
    threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not failures, failures


def test_the_gpu_list_leaves_no_family_out():
    count = collections.Counter(c.family for c in CASES)
    print(dict(count))
    assert set(count) == {c.family for c in tc.cases(random_tables=8)} and count["random tables"] >= 2000
    assert sum(tc.is_large(c) for c in CASES) >= 9
