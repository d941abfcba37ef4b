"""The device table reader's safety rule, without a GPU: whatever the grammar accepts, pandas reads to the same bits.

oracle/table.py (a plain model of cyto_table_read + cyto_table_fetch; token values from the host compilation of the converter)
is run on every file of tools/table_cases.py up to 16 MiB.  A file the model refuses must be refused with the triple (kind, line,
byte) that the generator planted; a file it accepts goes through common._table_frame -- the code that builds the user's DataFrame
from the device's arrays -- and must be equal to read_file(path): frame, dtypes, float bits (or be refused for its row labels).
tests/test_read_table_boundaries_gpu.py then holds the kernels to the same model, word for word."""
import collections
import time

import numpy as np
import pandas as pd
import pytest

from oracle.table import KIND_NAMES, table_model
from tools import table_cases as tc

CASES = tc.cases()
SMALL = [c for c in CASES if not tc.is_large(c)]
FAMILIES = sorted({c.family for c in SMALL})


def _equal(a, b):
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    for c in range(a.shape[1]):
        x, y = a.iloc[:, c].to_numpy(), b.iloc[:, c].to_numpy()
        assert x.dtype == y.dtype
        if x.dtype == np.float64:
            assert np.array_equal(x.view(np.int64), y.view(np.int64))


def _path(tmp_path, case):
    return tmp_path / (case.name + (".csv" if case.sep == b"," else ".tsv"))


def check_case(case, path):
    """One case through the model and, if accepted, through _table_frame against read_file.  Returns "refused", "equal" or
    "row labels"."""
    from cytospace_amd.common import _table_frame, _table_head, read_file
    data = case.make()
    path.write_bytes(data)
    d0, C = tc.header_end(data), tc.ncols_of(case, data)
    m = table_model(data, case.sep, d0, C)
    if case.intended != "device":
        assert m["status"] == 7 and m["reason"] == case.intended, (case.name, m.get("reason"), case.intended)
        return "refused"
    assert m["status"] == 0, (case.name, m.get("reason"))
    sep = case.sep.decode()
    header = data[:d0]
    first = data[d0:].split(b"\n", 1)[0] + b"\n"
    head = _table_head(header, first, sep, C)
    assert head is not None, case.name
    info = {}
    got = _table_frame(head, m["values"], m["is_float"], m["labels"], sep, info)
    if got is None:
        assert info["reason"]["kind"] == "row labels", (case.name, info)
        return "row labels"
    _equal(got, read_file(str(path)))
    return "equal"


@pytest.mark.parametrize("family", FAMILIES)
def test_model_gives_the_intended_refusal_or_pandas_frame(tmp_path, family):
    t = time.perf_counter()
    seen = collections.Counter()
    failed = []                                         # every case runs: a regression shows its whole pattern in one run
    for case in SMALL:
        if case.family == family:
            p = _path(tmp_path, case)
            try:
                seen[check_case(case, p)] += 1
            except Exception as e:                      # (AssertionError included)
                failed.append((case.name, repr(e)[:300]))
            p.unlink(missing_ok=True)
    n = sum(seen.values()) + len(failed)
    print(f"{family}: {n} cases {dict(seen)} in {time.perf_counter() - t:.1f} s")
    assert not failed, (len(failed), failed[:20])
    assert n == sum(c.family == family for c in SMALL) and n > 0
    # row labels outside the grammar are a refusal of their own; the families are built to stay clear of it but for a few labels
    assert seen["row labels"] <= max(2, n // 20), seen


def test_every_case_is_listed_and_has_an_outcome():
    count = collections.Counter(c.family for c in CASES)
    print(dict(count))
    assert count["random tables"] >= 2000 and count["one defect"] + count["two defects"] + count["host checks"] >= 140
    assert all(c.intended == "device" or (len(c.intended) == 3 and c.intended[0] in KIND_NAMES) for c in CASES)
    kinds = collections.Counter(c.intended[0] for c in CASES if c.intended != "device")
    assert set(kinds) == set(range(2, 10)) and min(kinds.values()) >= 15, kinds
    assert sum(tc.is_large(c) for c in CASES) <= 12


def test_the_two_writings_of_the_model_agree(tmp_path):
    """table_model walks a small file's lines in Python and searches arrays for a large one: the same result either way."""
    n = 0
    for case in SMALL:
        if case.family in ("random tables", "tokens", "column types", "long lines") and case.name != tc.MILLION:
            if case.family == "random tables" and int(case.name.split("_")[1]) % 10:
                continue
        elif case.family not in ("one defect", "two defects", "rounds", "host checks"):
            continue
        data = case.make()
        d0, C = tc.header_end(data), tc.ncols_of(case, data)
        a, b = table_model(data, case.sep, d0, C, vectorised=False), table_model(data, case.sep, d0, C, vectorised=True)
        assert a["status"] == b["status"], case.name
        if a["status"]:
            assert a["reason"] == b["reason"], case.name
        else:
            assert all(np.array_equal(a[k], b[k]) for k in ("values", "is_float", "labels")) and (a["G"], a["C"]) == (b["G"], b["C"])
        n += 1
    assert n > 300
