"""CPU tests (no GPU) of the text writers' fractional values (CYTO_TEXT_FRACTIONS; csrc/shortest.h, mtx.hip, csv.hip): the host hooks
run the functions the device's count and format passes call.  The power-of-ten table against Python integers; the shortest digits
against repr(float) and numpy's format_float_scientific(unique=True); cyto_mtx_format_entries_ex and cyto_csv_format_fields_ex byte
for byte against what scipy.io.mmwrite and DataFrame.to_csv write for the same values at run time; the flag's rules; and the host
side of write_mtx_device(fractions=True), which must not narrow a float64 matrix of fractions to float32."""
import ctypes
from decimal import Decimal

import numpy as np
import pandas as pd
import pytest

from _text_values import (BAD_ARG, CODES, FRACTIONS, UNSUPPORTED, all_values, edge_values, form_switch, pandas_fields_text, random_bits,
                          scipy_body)

NRANDOM = 1_000_000


def shortest(values):
    from cytospace_amd import _lib
    values = np.ascontiguousarray(values)
    n = len(values)
    digits, exp10 = np.zeros(n, np.uint64), np.zeros(n, np.int32)
    assert _lib.lib().cyto_shortest_digits(values.ctypes.data, CODES[values.dtype], n, digits.ctypes.data, exp10.ctypes.data) == 0
    return digits, exp10


def from_text(texts):
    """(digits without trailing zeros, exp10) of decimal texts, by decimal.Decimal."""
    digits, exp10 = np.zeros(len(texts), np.uint64), np.zeros(len(texts), np.int32)
    for i, s in enumerate(texts):
        _, d, e = Decimal(s).as_tuple()
        m = int("".join(map(str, d)))
        while m and m % 10 == 0:
            m //= 10
            e += 1
        digits[i], exp10[i] = m, e if m else 0
    return digits, exp10


def assert_digits(values, texts):
    got_d, got_e = shortest(values)
    want_d, want_e = from_text(texts)
    bad = np.flatnonzero((got_d != want_d) | (got_e != want_e))
    assert bad.size == 0, [(values[i], texts[i], int(got_d[i]), int(got_e[i])) for i in bad[:5]]
    assert int(got_d.max()) < (10**9 if values.dtype == np.float32 else 10**17)


def mtx_lines(values, flags=FRACTIONS):
    """(status, the text of all entry lines "i 1 value", offsets) of cyto_mtx_format_entries_ex for the n x 1 matrix of values."""
    from cytospace_amd import _lib
    values = np.ascontiguousarray(values)
    n = len(values)
    rows, cols = np.arange(n, dtype=np.int64), np.zeros(n, np.int64)
    out, off = np.zeros(64 * n + 1, np.uint8), np.zeros(n + 1, np.int64)
    st = _lib.lib().cyto_mtx_format_entries_ex(rows.ctypes.data, cols.ctypes.data, values.ctypes.data, CODES[values.dtype], n,
                                               out.ctypes.data, off.ctypes.data, flags)
    return st, out[:off[n]].tobytes() if st == 0 else None, off


def csv_fields(values, flags=FRACTIONS, cap=None):
    """(status, the fields each followed by a newline, lens) of cyto_csv_format_fields_ex."""
    from cytospace_amd import _lib
    values = np.ascontiguousarray(values)
    n = len(values)
    cap = 24 * n if cap is None else cap
    out, lens = np.zeros(cap + 1, np.uint8), np.zeros(n + 1, np.int32)
    st = _lib.lib().cyto_csv_format_fields_ex(values.ctypes.data, CODES[values.dtype], n, out.ctypes.data, cap, lens.ctypes.data, flags)
    if st:
        return st, None, lens[:n]
    lens = lens[:n].astype(np.int64)
    assert np.all(lens > 0) and lens.sum() <= cap
    ends = np.cumsum(lens)
    text = np.full(ends[-1] + n, ord("\n"), np.uint8)                      # field i moves right by i: a newline follows each
    keep = np.ones(len(text), bool)
    keep[ends + np.arange(n)] = False
    text[keep] = out[:ends[-1]]
    return st, text.tobytes(), lens


def first_difference(got, want):
    a, b = got.split(b"\n"), want.split(b"\n")
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, x, y
    return min(len(a), len(b)), len(a), len(b)


def assert_mtx(values):
    st, got, _ = mtx_lines(values)
    assert st == 0
    want = scipy_body(values)
    assert got == want, first_difference(got, want)
    return got


def assert_csv(values):
    st, got, lens = csv_fields(values)
    assert st == 0
    want = pandas_fields_text(values)
    assert got == want, first_difference(got, want)
    return got, lens


def test_every_power_of_ten_of_the_table_equals_python_integers():
    from cytospace_amd import _lib
    out = np.zeros(2, np.uint64)
    for k in range(-292, 325):
        assert _lib.lib().cyto_text_pow10(k, out.ctypes.data) == 0
        if k >= 0:
            p = 10**k
            sh = p.bit_length() - 128
            want = p << -sh if sh <= 0 else -((-p) >> sh)
            assert (want << max(sh, 0)) >= (p << max(-sh, 0)) > ((want - 1) << max(sh, 0))       # the ceiling of p / 2^sh
        else:
            d = 10**-k
            sh = 127 + d.bit_length()
            want = -((-(1 << sh)) // d)
            assert want * d >= (1 << sh) > (want - 1) * d
        assert (1 << 127) <= want < (1 << 128)
        assert (int(out[0]) << 64) | int(out[1]) == want, k
    for k in (-293, 325):
        assert _lib.lib().cyto_text_pow10(k, out.ctypes.data) == BAD_ARG


def test_the_committed_table_is_what_its_generator_writes():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools")
    sys.path.insert(0, tools)
    try:
        import gen_pow10_table
    finally:
        sys.path.remove(tools)
    with open(gen_pow10_table.OUT) as f:
        assert f.read() == gen_pow10_table.text()


def test_float64_digits_equal_repr_on_a_million_bit_patterns():
    v = np.abs(random_bits(np.float64, NRANDOM, 1))
    v = v[v > 0]
    assert_digits(v, [repr(x) for x in v.tolist()])


def test_float32_digits_equal_numpy_on_a_million_bit_patterns():
    v = np.abs(random_bits(np.float32, NRANDOM, 2))
    v = v[v > 0]
    texts = v.astype(str)                      # numpy's shortest digits of a float32, vectorised; the scalar routine is pinned below
    probe = from_text([np.format_float_scientific(x, unique=True) for x in v[:2000]])
    assert all(np.array_equal(a, b) for a, b in zip(from_text(texts[:2000].tolist()), probe))
    assert_digits(v, texts.tolist())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_digits_at_the_binade_edges_powers_of_ten_subnormals_and_every_digit_count(dtype):
    v = np.concatenate([edge_values(dtype), form_switch(dtype)])
    v = v[v > 0]
    if dtype == np.float64:
        texts = [repr(x) for x in v.tolist()]
    else:
        texts = [np.format_float_scientific(x, unique=True) for x in v]
    assert_digits(v, texts)
    d, e = shortest(np.array([0.0, -0.0, -2.5], dtype))                      # a zero is (0, 0); the sign is ignored
    assert d.tolist() == [0, 0, 25] and e.tolist() == [0, 0, -1]
    fi = np.finfo(dtype)
    d, e = shortest(np.array([fi.smallest_subnormal, fi.max], dtype))
    assert (d.tolist(), e.tolist()) == (([1, 34028235], [-45, 31]) if dtype == np.float32 else ([5, 17976931348623157], [-324, 292]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_digits_hook_rejects_what_it_does_not_take(dtype):
    from cytospace_amd import _lib
    d, e = np.zeros(2, np.uint64), np.zeros(2, np.int32)
    for bad in (np.nan, np.inf, -np.inf):
        v = np.array([1.5, bad], dtype)
        assert _lib.lib().cyto_shortest_digits(v.ctypes.data, CODES[v.dtype], 2, d.ctypes.data, e.ctypes.data) == BAD_ARG
    v = np.array([1, 2], np.int32)
    assert _lib.lib().cyto_shortest_digits(v.ctypes.data, CODES[v.dtype], 2, d.ctypes.data, e.ctypes.data) == BAD_ARG


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mtx_entries_equal_scipy(dtype):
    got = assert_mtx(all_values(dtype, NRANDOM))
    assert b" 1 1E-1\n" in assert_mtx(np.array([0.0, 0.1, -0.0, 2.5, 250.0, 10.0, -1.234e-4], dtype))


def test_mtx_examples_and_the_longest_texts():
    v = np.array([0.1, 2.5, 1 / 3, 5e-324, 1.7976931348623157e308, 1.234e-4, 9.999999999999998e15, 250.0, 10.0, -1.7976931348623157e308,
                  -2.2250738585072014e-308, 2.0**53, 2.0**53 - 1, 2.0**53 + 2, 1e22, 1e23], np.float64)
    got = assert_mtx(v).split(b"\n")
    values = [g.split(b" ")[2] for g in got[:-1]]
    assert values[:9] == [b"1E-1", b"2.5", b"3.333333333333333E-1", b"5E-324", b"1.7976931348623157E308", b"1.234E-4", b"9.999999999999998E15",
                          b"2.5E2", b"1E1"]
    assert values[9] == b"-1.7976931348623157E308" and values[10] == b"-2.2250738585072014E-308" and len(values[10]) == 24
    v = np.array([0.1, 1 / 3, 2.0**24, 2.0**24 - 1, 2.0**24 + 2, 1e-45, 3.4028235e38, -1.1754944e-38], np.float32)
    values = [g.split(b" ")[2] for g in assert_mtx(v).split(b"\n")[:-1]]
    assert values[:2] == [b"1E-1", b"3.3333334E-1"] and values[-1] == b"-1.1754944E-38"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_csv_fields_equal_pandas(dtype):
    v = all_values(dtype, NRANDOM)
    got, lens = assert_csv(v)
    assert int(lens.max()) == 24 if dtype == np.float64 else int(lens.max()) <= 19
    assert_csv(np.array([0.0, -0.0, 0.1, 2.5, 250.0, 10.0, -1.234e-4], dtype))


def test_csv_examples_the_form_switch_and_the_longest_texts():
    v = np.array([1e-4, 1 / 3, 2.5, 1000000000000000.5, 9999999999999998.0, 9007199254740992.0, 1e-5, 1e16, 1.5e20, 5e-324, 1.7976931348623157e308,
                  0.0, -0.0, -1.7976931348623157e308, -2.2250738585072014e-308, -0.00012345678901234567, 9.999999999999999e-5, 123456.789], np.float64)
    got, lens = assert_csv(v)
    assert got.split(b"\n")[:-1] == [b"0.0001", b"0.3333333333333333", b"2.5", b"1000000000000000.5", b"9999999999999998.0", b"9007199254740992.0",
                                     b"1e-05", b"1e+16", b"1.5e+20", b"5e-324", b"1.7976931348623157e+308", b"0.0", b"-0.0",
                                     b"-1.7976931348623157e+308", b"-2.2250738585072014e-308", b"-0.00012345678901234567", b"9.999999999999999e-05",
                                     b"123456.789"]
    assert int(lens.max()) == 24
    # float32: the switch is on the value.  The edge itself comes from the library on this machine.
    edge = np.array([1e-4], np.float32)
    below, above = np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1))
    v = np.concatenate([below, edge, above, np.array([1 / 3, 1.2345679e17, -9999999000000000.0, 1e16, 16777216.0, 16777218.0, 0.1], np.float32)])
    got, lens = assert_csv(v)
    fields = got.split(b"\n")[:-1]
    assert fields[1] == pandas_fields_text(edge)[:-1] and fields[3:6] == [b"0.33333334", b"1.2345679e+17", b"-9999999000000000.0"]
    assert int(lens.max()) == 19
    got, lens = assert_csv(form_switch(np.float32))
    assert b"e-" in got and b"0.000" in got and b"e+16" in got and b"00000000.0\n" in got           # both forms on both sides
    got, lens = assert_csv(form_switch(np.float64))
    assert b"e-05" in got and b"0.0001" in got and b"e+16" in got and b"9999999999999998.0\n" in got


def refused_values(dtype):
    lim = 2.0**24 if dtype == np.float32 else 2.0**53
    return [(2, 2.5), (2, 0.1), (2, -1e-30), (4, lim), (4, -lim * 4), (3, np.nan), (3, np.inf), (3, -np.inf)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_flags_zero_is_the_old_hooks_on_refused_and_taken_values(dtype):
    from cytospace_amd import _lib
    L = _lib.lib()
    for kind, bad in refused_values(dtype):
        v = np.array([3.0, -0.0, 1200.0, bad, 7.0], dtype)
        n = len(v)
        st, _, lens = csv_fields(v, flags=0, cap=20 * n)
        out, old = np.zeros(20 * n, np.uint8), np.zeros(n, np.int32)
        assert L.cyto_csv_format_fields(v.ctypes.data, CODES[v.dtype], n, out.ctypes.data, 20 * n, old.ctypes.data) == UNSUPPORTED == st
        assert lens.tolist() == old.tolist() and lens[3] == -kind
        st, _, off = mtx_lines(v, flags=0)
        rows, cols = np.arange(n, dtype=np.int64), np.zeros(n, np.int64)
        out, old = np.zeros(64 * n, np.uint8), np.zeros(n + 1, np.int64)
        assert L.cyto_mtx_format_entries(rows.ctypes.data, cols.ctypes.data, v.ctypes.data, CODES[v.dtype], n, out.ctypes.data,
                                         old.ctypes.data) == UNSUPPORTED == st
        assert off.tolist() == old.tolist()
    v = np.array([3.0, -0.0, 1200.0, -16777215.0, 0.0], dtype)                # taken: the same bytes with and without the flag
    assert csv_fields(v, flags=0, cap=20 * len(v))[1] == csv_fields(v)[1] == pandas_fields_text(v)
    assert mtx_lines(v, flags=0)[1] == mtx_lines(v)[1] == scipy_body(v)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_under_the_flag_only_non_finite_values_are_refused(dtype):
    for kind, bad in refused_values(dtype):
        v = np.array([3.0, 0.25, bad, 7.0], dtype)
        st, _, lens = csv_fields(v)
        st_m, _, _ = mtx_lines(v)
        if kind == 3:
            assert st == UNSUPPORTED and lens[2] == -3 and lens[1] == 4 and st_m == UNSUPPORTED         # CYTO_CSV_ERR_NONFINITE
        else:
            assert st == 0 and st_m == 0


def test_unknown_flag_bits_and_a_short_buffer_are_bad_arguments():
    v = np.array([1.0, 2.5], np.float64)
    for flags in (2, 3, 4, -1, 1 << 30):
        assert csv_fields(v, flags=flags)[0] == BAD_ARG and mtx_lines(v, flags=flags)[0] == BAD_ARG
    assert csv_fields(v, cap=47)[0] == BAD_ARG and csv_fields(v, cap=48)[0] == 0 and csv_fields(v, flags=0, cap=40)[0] == UNSUPPORTED
    from cytospace_amd import _lib
    info, cinfo = _lib.MtxInfo(), _lib.CsvInfo()
    cols, off = np.zeros(1, np.int64), np.zeros(3, np.int64)
    x = np.ones((2, 1))
    for flags in (2, 5, -1):                   # (before any device is touched: this test has none)
        assert _lib.lib().cyto_mtx_write_ex(b"/nonexistent/m", 2, 1, x.ctypes.data, 1, 1, cols.ctypes.data, 1, 0, 0, flags, ctypes.byref(info)) == BAD_ARG
        assert _lib.lib().cyto_csv_write_ex(b"/nonexistent/c", 2, 1, x.ctypes.data, 1, 1, cols.ctypes.data, 1, b",a\n", 3, b"", off.ctypes.data, 0, 0,
                                            flags, ctypes.byref(cinfo)) == BAD_ARG


def test_integer_types_are_the_same_with_and_without_the_flag():
    for dtype in (np.uint8, np.uint16, np.int32, np.int64):
        ii = np.iinfo(dtype)
        v = np.array([0, 1, 10, 250, ii.max, ii.min, ii.max // 3], dtype)
        assert csv_fields(v)[1] == csv_fields(v, flags=0)[1] == pandas_fields_text(v)
        assert mtx_lines(v)[1] == mtx_lines(v, flags=0)[1]


class _Stub:
    """The library as write_mtx_device sees it: records what it is handed."""
    def __init__(self):
        self.calls = []

    def cyto_mtx_write_ex(self, path, G, N, x, ldx, code, cols, C, block_bytes, device_id, flags, info):
        self.calls.append(("ex", code, flags))
        return 0

    def cyto_mtx_write(self, path, G, N, x, ldx, code, cols, C, block_bytes, device_id, info):
        self.calls.append(("plain", code, 0))
        return 0


def test_write_mtx_device_with_fractions_narrows_only_all_integer_frames(monkeypatch, tmp_path):
    from cytospace_amd import _lib, post_processing
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    rng = np.random.default_rng(4)
    ints = rng.poisson(2.0, (6, 9)).astype(np.float64)
    exact32 = ints.copy()
    exact32[2, 3] = 0.5                                                       # float32-exact, and 0.5 in either type
    trap = ints.copy()
    trap[4, 1] = float(np.float32(0.1))                                       # float32-exact; 0.10000000149011612 as a float64
    cols = [0, 2, 8, 8]
    path = str(tmp_path / "m.mtx")
    for frame in (ints, pd.DataFrame(ints)):
        post_processing.write_mtx_device(path, frame, cols, fractions=True)
        assert stub.calls.pop() == ("ex", _lib.CYTO_DTYPE_F32, _lib.CYTO_TEXT_FRACTIONS)
    for x in (exact32, trap, pd.DataFrame(trap)):
        post_processing.write_mtx_device(path, x, cols, fractions=True)
        assert stub.calls.pop() == ("ex", _lib.CYTO_DTYPE_F64, _lib.CYTO_TEXT_FRACTIONS)
    for x in (ints, exact32, trap):                                           # the default path narrows as before
        post_processing.write_mtx_device(path, x, cols)
        assert stub.calls.pop() == ("plain", _lib.CYTO_DTYPE_F32, 0)
    post_processing.write_mtx_device(path, ints.astype(np.float32) + np.float32(0.25), cols, fractions=True)
    assert stub.calls.pop() == ("ex", _lib.CYTO_DTYPE_F32, _lib.CYTO_TEXT_FRACTIONS)
    assert stub.calls == []


def test_save_results_passes_fractions_to_both_device_writers(monkeypatch, tmp_path):
    from cytospace_amd import post_processing
    seen = {}
    monkeypatch.setattr(post_processing, "write_mtx_device", lambda path, frame, columns, **kw: seen.__setitem__("mtx", kw))
    monkeypatch.setattr(post_processing, "write_csv_device", lambda path, frame, columns, **kw: seen.__setitem__("csv", kw))
    expr = pd.DataFrame(np.arange(12.0).reshape(3, 4) / 8, index=["GENE_a", "GENE_b", "GENE_c"],
                        columns=["CELL_1", "CELL_2", "CELL_B_new_1", "CELL_B_new_2"])
    ctd = pd.DataFrame({"CellType": ["TYPE_B", "TYPE_B"]}, index=["CELL_1", "CELL_2"])
    assigned = pd.DataFrame({"row": [1, 2], "col": [3, 4]}, index=["SPOT_a", "SPOT_b"])
    post_processing.save_results(str(tmp_path), "p_", np.array(["CELL_1", "CELL_2"]), expr, assigned, ctd, "duplicates", True, device_id=0)
    post_processing.save_results(str(tmp_path), "q_", np.array(["CELL_B_new_1", "CELL_B_new_2"]), expr, assigned, ctd, "place_holders", True,
                                 device_id=0)
    assert seen["mtx"]["fractions"] is True and seen["csv"]["fractions"] is True
