"""The device table reader's decimal converter (csrc/table.hip: parse_token, run on the host through cyto_table_parse_tokens)
against pandas' own: 10^6 random tokens read by pd.read_csv as float64, compared bit for bit, and the integer tokens as int64."""
import io

import numpy as np
import pandas as pd


def _tokens(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    digits = rng.integers(0, 10, (n, 24)).astype(str)
    for i in range(n):
        form = i % 6
        nd = int(rng.integers(1, 25))
        ds = "".join(digits[i, :nd])
        if form == 0:                                   # 1-24 digits, a point somewhere, an exponent -300..280
            p = int(rng.integers(0, nd + 1))
            t = ds[:p] + "." + ds[p:] if rng.random() < 0.8 else ds
            if rng.random() < 0.7:
                t += f"{'eE'[i & 1]}{int(rng.integers(-300, 281)):+d}"
        elif form == 1:                                 # long zero runs after the point
            t = "0." + "0" * int(rng.integers(0, 40)) + ds[:int(rng.integers(1, 12))]
        elif form == 2:                                 # 17-24 digit mantissas
            t = "".join(digits[i, :int(rng.integers(17, 25))]).lstrip("0") or "0"
            t = t + "." + ds[:3] if rng.random() < 0.5 else t + "e" + str(int(rng.integers(-20, 20)))
        elif form == 3:                                 # below 1e-308: the two-step division, and below 1e-616
            t = ds[:int(rng.integers(1, 18))] + "e" + str(int(rng.integers(-340, -300)) if rng.random() < 0.9 else -700)
        elif form == 4:                                 # integer tokens of 1-18 digits
            t = ds[:int(rng.integers(1, 19))]
        else:                                           # short decimals, as written by R or to_csv
            t = f"{rng.normal() * 10 ** int(rng.integers(-6, 7)):.{int(rng.integers(0, 9))}f}"
        if rng.random() < 0.3 and not t.startswith("-"):
            t = ("-" if rng.random() < 0.7 else "+") + t
        if len(t.lstrip("+-")) > 18 and t.lstrip("+-").isdigit():
            t += "."                                    # (a digit string of 19+ digits is no decimal token: pandas reads it as an integer)
        out.append(t)
    return out


SPECIAL = ["-0", "-0.0", "5.", ".5", "007", "0", "+0", "0.0", "-.5", "999999999999999999", "-999999999999999999",
           "000000000000000012", "0.000000000000000000000000001", "1.7976931348623157e308", "4.9e-324", "2.2250738585072011e-308",
           "123456789012345678901234.", "-1e-700", "1e-330", "9.999999999999999999e-309"]


def _pandas_floats(tokens):
    return pd.read_csv(io.StringIO("\n".join(tokens)), header=None, dtype=np.float64)[0].to_numpy()


def test_converter_equals_pandas_on_a_million_tokens():
    from cytospace_amd.common import parse_table_tokens
    toks = SPECIAL + _tokens(1_000_000)
    kind, value, ints = parse_table_tokens(toks)
    assert set(np.unique(kind)) <= {0, 1}, [t for t, k in zip(toks, kind) if k > 1][:5]
    want = _pandas_floats(toks)
    bad = np.flatnonzero(value.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, [(toks[i], value[i], want[i]) for i in bad[:10]]
    isint = kind == 0
    assert isint.sum() > 100_000
    want_int = pd.read_csv(io.StringIO("\n".join(np.asarray(toks, dtype=object)[isint])), header=None, dtype=np.int64)[0].to_numpy()
    assert np.array_equal(ints[isint], want_int)


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
