"""The device table reader's decimal converter (csrc/table.hip: parse_token, run on the host through cyto_table_parse_tokens)
against pandas' own: 10^6 random tokens read by pd.read_csv as float64, compared bit for bit, and the integer tokens as int64;
and the tokens that are numbers but outside the grammar."""
import io

import numpy as np
import pandas as pd

from tools.table_cases import SPECIAL, in_grammar, random_tokens as _tokens     # (shared with the table files of the model tests)


def _pandas_floats(tokens):
    return pd.read_csv(io.StringIO("\n".join(tokens)), header=None, dtype=np.float64)[0].to_numpy()


def test_converter_equals_pandas_on_a_million_tokens():
    from cytospace_amd.common import parse_table_tokens
    toks = SPECIAL + _tokens(1_200_000)
    kind, value, ints = parse_table_tokens(toks)
    inside = np.array([in_grammar(t) for t in toks])     # (more than 18 digits before the point: see the test below)
    assert (kind[~inside] == 2).all() and (~inside).sum() > 100_000
    toks, kind, value, ints = [t for t, k in zip(toks, inside) if k], kind[inside], value[inside], ints[inside]
    assert len(toks) >= 1_000_000
    assert set(np.unique(kind)) <= {0, 1}, [t for t, k in zip(toks, kind) if k > 1][:5]
    want = _pandas_floats(toks)
    bad = np.flatnonzero(value.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, [(toks[i], value[i], want[i]) for i in bad[:10]]
    isint = kind == 0
    assert isint.sum() > 100_000
    want_int = pd.read_csv(io.StringIO("\n".join(np.asarray(toks, dtype=object)[isint])), header=None, dtype=np.int64)[0].to_numpy()
    assert np.array_equal(ints[isint], want_int)


def test_decimal_tokens_with_more_than_18_integer_digits_are_outside_the_grammar():
    # pandas tries a column as int64, then uint64, before float64; digits beyond uint64 met before a token with a point or an
    # exponent end that attempt with an overflow, and the column stays text.  So the order of a column's tokens decides its type,
    # and the reader leaves every such token to pandas: 18 digits can overflow neither int64 nor uint64.
    from cytospace_amd.common import parse_table_tokens
    assert pd.read_csv(io.StringIO("a\n7\n56963997270084518163.5\n"))["a"].dtype == object
    assert pd.read_csv(io.StringIO("a\n18446744073709551616e0\n0.5\n"))["a"].dtype == object
    assert pd.read_csv(io.StringIO("a\n0.5\n56963997270084518163.5\n"))["a"].dtype == np.float64
    assert pd.read_csv(io.StringIO("a\n7\n999999999999999999.5\n-999999999999999999e1\n"))["a"].dtype == np.float64
    kind, _, _ = parse_table_tokens(["56963997270084518163.5", "18446744073709551616e0", "1234567890123456789.", "-1234567890123456789e-30",
                                     "0000000000000000000.5", "999999999999999999.5", "-999999999999999999e1", "123456789012345678."])
    assert list(kind) == [2, 2, 2, 2, 2, 1, 1, 1]


def test_special_tokens():
    from cytospace_amd.common import parse_table_tokens
    kind, value, ints = parse_table_tokens(SPECIAL)
    got = dict(zip(SPECIAL, zip(kind, value, ints)))
    assert got["-0"][0] == 0 and got["-0"][2] == 0 and np.signbit(got["-0"][1])
    assert got["-0.0"][0] == 1 and np.signbit(got["-0.0"][1])
    assert got["5."][1] == 5.0 and got[".5"][1] == 0.5 and got["007"][2] == 7
    assert got["999999999999999999"][2] == 10**18 - 1 and got["-999999999999999999"][2] == -(10**18 - 1)
    assert got["000000000000000012"][1] == 10.0          # pandas: the 17 digits kept include the leading zeros
    assert got["0.000000000000000000000000001"][1] == 0.0


def test_tokens_outside_the_grammar():
    from cytospace_amd.common import parse_table_tokens
    bad = ["", "-", "+", ".", "NA", "nan", "inf", "1e", "1e+", "1e12345", "1.2.3", "1,5", " 1", "1 ", "0x10", "1_000", "--1",
           "1234567890123456789", "0000000000000000001"]
    kind, _, _ = parse_table_tokens(bad)
    assert (kind == 2).all(), [t for t, k in zip(bad, kind) if k != 2]
    rng = ["1e400", "-1e309", "2e308", "9e308", "1e309"]
    kind, _, _ = parse_table_tokens(rng)
    assert (kind == 3).all()
    for t in rng:                       # pandas keeps such a column as text
        assert pd.read_csv(io.StringIO("a\n" + t + "\n"))["a"].dtype == object
