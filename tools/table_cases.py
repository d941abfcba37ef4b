"""Seeded files for the device table reader (csrc/table.hip), each with its intended outcome, shared by
tests/test_read_table_model_cpu.py and tests/test_read_table_boundaries_gpu.py.

A Case knows its bytes (`make()`, deterministic: PCG64 seeds), its delimiter, the `ncols` and `data_offset` to read it with, and
what it was built to be: "device" (inside the grammar of DESIGN.md 4.1c) or the refusal (kind, line, byte) that the generator
knows FROM CONSTRUCTION -- it planted the defect and kept its position -- never from the model or the reader.  Every boundary
family asserts its geometry on the bytes it wrote (`check`), so a case cannot quietly stop testing the edge it is named after.

The numbers below are the kernels' (table.hip): tbl_lines takes a workgroup per 64 KiB block and a thread per 256 bytes;
tbl_fields takes a thread per 16-byte slice, counted from the line's start rounded down to 16, 256 slices (4 KiB) per round; the
upload goes in 16 MiB chunks; tbl_scan_blocks scans 256 block counts per pass.

`python -m tools.table_cases` prints the number of cases per family."""
import collections
import functools

import numpy as np

BLOCK, SPAN, SLICE, ROUND, CHUNK = 65536, 256, 16, 4096, 16 << 20
BYTE, QUOTE, CR, BLANK, FIELDS, TOKEN, RANGE, INT_CAST = 2, 3, 4, 5, 6, 7, 8, 9         # CYTO_TABLE_ERR_* (include/cytohip.h)
LARGE = 16 << 20                # files above this are read on the GPU only, against the model only

Case = collections.namedtuple("Case", "name family make sep ncols intended")


def header_end(data):
    """data_offset as common._table_on_device finds it: the byte after the first '\\n'."""
    head = bytes(data[:1 << 20])
    return head.index(b"\n") + 1


# ---- tokens ----------------------------------------------------------------------------------------------------------------

def random_tokens(n, seed=0):
    """n tokens of the reader's grammar in six forms (the converter tests' set)."""
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
# (pandas gives 1e5, 1e5, 0.0, -50.0, 0.0, 1.0)
EXTRA = ["1.e5", "1e0005", "1e-0400", "-.5e+2", "0." + "0" * 3997 + "5", "1." + "0" * 3998]


def is_integer_token(t):
    return t.lstrip("+-").isdigit()


def int_digits(t):
    """The digits of a token before its point or exponent."""
    d = t.lstrip("+-")
    return len(d) - len(d.lstrip("0123456789"))


def in_grammar(t):
    """random_tokens, SPECIAL and EXTRA hold numbers only; of those the grammar leaves out the ones with more than 18 digits
    before the point (pandas may keep their column as text)."""
    return int_digits(t) <= 18


def _safe_in_float_column(t):
    """An integer token that may stand in a float64 column: at most 16 digits and no negative zero."""
    d = t.lstrip("+-")
    return len(d) <= 16 and not (t.startswith("-") and int(d) == 0)


_pool_cache = {}


def token_pool(n=120_000, seed=77):
    """(integer tokens, decimal tokens) to draw small tables from: every form of random_tokens, SPECIAL and EXTRA's short ones."""
    if (n, seed) not in _pool_cache:
        toks = [t for t in random_tokens(n, seed) + SPECIAL * 50 + EXTRA[:4] * 50 if in_grammar(t)]
        _pool_cache[(n, seed)] = ([t for t in toks if is_integer_token(t)], [t for t in toks if not is_integer_token(t)])
    return _pool_cache[(n, seed)]


# ---- assembling a file and keeping positions --------------------------------------------------------------------------------

class _File:
    """A table under construction: the header, then data lines; `pos` is where the next line starts."""

    def __init__(self, sep=b"\t", eol=b"\n", ncols=3, header=None, r_header=False):
        self.sep, self.eol, self.C = sep, eol, ncols
        if header is None:
            names = [b"c%d" % j for j in range(ncols)]
            header = sep.join(names if r_header else [b"ID"] + names) + eol
        self.parts = [header]
        self.pos = len(header)
        self.d0 = len(header)
        self.starts = []                                # where every data line starts

    def line_bytes(self, label, tokens):
        return label + b"".join(self.sep + t for t in tokens)

    def add(self, label, tokens=None, eol=None):
        """One data line; returns where it starts."""
        if tokens is None:
            tokens = [b"1"] * self.C
        raw = self.line_bytes(label, tokens) + (self.eol if eol is None else eol)
        return self.add_raw(raw)

    def add_raw(self, raw):
        self.starts.append(self.pos)
        self.parts.append(raw)
        self.pos += len(raw)
        return self.starts[-1]

    def min_line(self):
        return 1 + 2 * self.C + len(self.eol)

    def fill_to(self, target, lo=40, hi=90):
        """Ordinary short lines (labels g<n>xxx..., values 1) until the next line starts exactly at `target`."""
        assert target == self.pos or target - self.pos >= self.min_line(), (target, self.pos)
        k = 0
        while self.pos < target:
            left = target - self.pos
            n = left if left < hi + self.min_line() + 10 else lo + (k * 7) % (hi - lo)
            if left - n < self.min_line() and left != n:
                n = left
            lab = n - 2 * self.C - len(self.eol)
            tag = b"g%d" % len(self.starts)
            self.add((tag + b"x" * lab)[:lab] if lab >= 1 else b"", None)
            k += 1
        assert self.pos == target
        return self

    def line_no(self, i=-1):
        """The file's line number (the header is line 1) of data line i."""
        return (len(self.starts) + i if i < 0 else i) + 2

    def data(self):
        return b"".join(self.parts)


def _case(name, family, make, sep, ncols, intended, check=None):
    """make() -> bytes; check(data) asserts the geometry the case is named after, every time the bytes are made."""
    def made():
        data = make()
        if check is not None:
            check(data)
        return data
    return Case(name, family, made, sep, ncols, intended)


# ---- inside the grammar ------------------------------------------------------------------------------------------------------

def _edge_cases(family, edges, eols=(b"\n",)):
    """A line end, a split CRLF, the data offset and the file's end at every offset of `edges`."""
    out = []
    for X in edges:
        def nl_at(X=X):
            f = _File()
            f.fill_to(X - 40).add(b"g" + b"e" * 33)                   # 40 bytes of text: this line's '\n' is byte X
            f.fill_to(X + 1 + 300)
            return f.data()
        out.append(_case(f"nl_at_{X}", family, nl_at, b"\t", 3, "device", lambda d, X=X: _assert(d[X:X + 1] == b"\n" and d[X - 1] != 13)))

        def crlf_at(X=X):
            f = _File(eol=b"\r\n")
            f.fill_to(X - 1 - 38).add(b"g" + b"e" * 31)               # 38 bytes of text: '\r' is byte X - 1, '\n' is byte X
            f.fill_to(X + 1 + 300)
            return f.data()
        out.append(_case(f"crlf_at_{X}", family, crlf_at, b"\t", 3, "device", lambda d, X=X: _assert(d[X - 1:X + 1] == b"\r\n")))

        def offset_at(X=X):
            names = [b"first", b"n" * (X - 15), b"last"]
            header = b"\t".join([b"ID"] + names) + b"\n"
            f = _File(header=header)
            assert f.d0 == X
            for g in range(5):
                f.add(b"g%d" % g, [b"%d" % (g + 1), b"0.5", b"7"])
            return f.data()
        out.append(_case(f"data_offset_{X}", family, offset_at, b"\t", 3, "device",
                         lambda d, X=X: _assert(header_end(d) == X and d[X - 1:X] == b"\n")))
        for final in (True, False):
            def ends_at(X=X, final=final):
                f = _File()
                tail = 30
                f.fill_to(X - tail)
                raw = f.line_bytes(b"z" * (tail - 6 - (1 if final else 0)), [b"1", b"2", b"3"]) + (b"\n" if final else b"")
                f.add_raw(raw)
                return f.data()
            out.append(_case(f"length_{X}_{'nl' if final else 'open'}", family, ends_at, b"\t", 3, "device",
                             lambda d, X=X, final=final: _assert(len(d) == X and (d[-1:] == b"\n") == final)))
    return out


def _assert(ok):
    assert ok


def _long_lines():
    out = []
    for n, name in ((70_000, "over_64k"), (140_000, "over_128k")):
        def make(n=n):
            f = _File()
            f.add(b"a")
            f.add(b"L" * n, [b"11", b"2.5", b"-3"])
            f.add(b"b", [b"4", b"5", b"6"])
            f.add(b"M" * (n + 4321), [b"7", b"8", b"9"])
            f.add(b"c")
            return f.data()
        out.append(_case(f"label_{name}", "long lines", make, b"\t", 3, "device",
                         lambda d, n=n: _assert(max(len(x) for x in d.split(b"\n")) > n)))

    def wide():
        rng = np.random.default_rng(70)
        C = 70_000
        rows = [b"ID\t" + b"\t".join(b"c%d" % j for j in range(C)) + b"\n"]
        for g in range(3):
            row = np.full(2 * C, 9, np.uint8)
            row[1::2] = 48 + rng.integers(0, 10, C)
            rows.append(b"gene%d" % g + row.tobytes() + b"\n")
        return b"".join(rows)
    out.append(_case("three_by_70000", "long lines", wide, b"\t", 70_000, "device",
                     lambda d: _assert(min(len(x) for x in d.split(b"\n")[1:4]) > 2 * BLOCK)))
    return out


def _slice_cases():
    out = []
    for k in range(16):                                 # line starts at s mod 16 == k; one such line for every e mod 16
        def make(k=k):
            f = _File(ncols=2)
            for j in range(16):
                f.fill_to(_next_congruent(f.pos + f.min_line(), k, 16))
                s = f.pos
                n = _next_congruent(s + 8, j, 16) - s                # the line's text is [s, s + n)
                f.add(b"w" * (n - 7), [b"12", b"3.5"])
            f.add(b"end")
            return f.data()

        def check(d, k=k):
            want = {(k, j) for j in range(16)}
            s = header_end(d)
            for ln in d[s:].split(b"\n")[:-1]:
                want.discard((s % 16, (s + len(ln)) % 16))
                s += len(ln) + 1
            assert not want, want
        out.append(_case(f"start_mod16_{k}", "slices", make, b"\t", 2, "device", check))
    for L in (1, 2, 15, 16, 17, 30):                    # a token of L bytes at every start mod 16: it straddles a slice edge
        tok = (b"1234567890123456789012345678901"[:L] if L < 19 else b"12345678901234.567890123456789012345"[:L])

        def make(L=L, tok=tok):
            f = _File(ncols=3)
            for r in range(16):
                f.fill_to(_next_congruent(f.pos + f.min_line(), 0, 16))
                f.add(b"q" * (15 + r), [b"8", tok, b"9"])          # the token starts at s + 15 + r + 3
            return f.data()

        def check(d, L=L, tok=tok):
            seen = set()
            s = header_end(d)
            for ln in d[s:].split(b"\n")[:-1]:
                if ln.startswith(b"q"):
                    p = s + ln.index(b"\t" + tok + b"\t") + 1
                    seen.add(p % 16)
                s += len(ln) + 1
            assert seen == set(range(16))
        out.append(_case(f"token_len_{L}", "slices", make, b"\t", 3, "device", check))
    return out


def _next_congruent(at_least, k, m):
    return at_least + (k - at_least) % m


def _round_cases():
    """Lines placed against the 4 KiB rounds of tbl_fields, which count from a0 = s rounded down to 16."""
    out = []
    for smod in (0, 5):
        def start(f, smod=smod):
            f.add(b"first")
            f.fill_to(_next_congruent(f.pos + f.min_line(), smod, 16))
            return f.pos, f.pos - smod                  # s, a0

        def delim_last(start=start):                    # a delimiter as the last byte of round 0, its token in round 1
            f = _File(ncols=3)
            s, a0 = start(f)
            f.add(b"r" * (a0 + ROUND - 1 - s - 2), [b"5", b"123456", b"7"])
            f.add(b"after")
            return f.data()

        def check_delim(d, smod=smod):
            s = d.index(b"\nr") + 1
            a0 = s - smod
            assert s % 16 == smod and d[a0 + ROUND - 1:a0 + ROUND + 6] == b"\t123456"
        out.append(_case(f"delimiter_ends_round_s{smod}", "rounds", delim_last, b"\t", 3, "device", check_delim))

        def token_over_edge(start=start):               # a 30-byte token that begins 13 bytes before the round's end
            f = _File(ncols=3)
            s, a0 = start(f)
            f.add(b"r" * (a0 + ROUND - 13 - s - 3), [b"5", b"12345678901234.567890123456789", b"7"])
            f.add(b"after")
            return f.data()

        def check_tok(d, smod=smod):
            s = d.index(b"\nr") + 1
            assert s % 16 == smod and d.index(b"\t12345678901234.5") + 1 == s - smod + ROUND - 13
        out.append(_case(f"token_over_round_edge_s{smod}", "rounds", token_over_edge, b"\t", 3, "device", check_tok))
        for n in (ROUND - 1, ROUND, ROUND + 1, 2 * ROUND - 1, 2 * ROUND, 2 * ROUND + 1):
            def exact(n=n, start=start):                # the line's text ends n bytes after a0
                f = _File(ncols=3)
                s, a0 = start(f)
                mid = (a0 + n - s) // 2
                f.add(b"r" * mid, [b"5", b"6." + b"0" * (a0 + n - s - mid - 7), b"7"])
                f.add(b"after")
                return f.data()

            def check_exact(d, n=n, smod=smod):
                s = d.index(b"\nr") + 1
                e = d.index(b"\n", s)
                assert s % 16 == smod and e - (s - smod) == n
            out.append(_case(f"line_of_{n}_s{smod}", "rounds", exact, b"\t", 3, "device", check_exact))

        def bare_last_round(start=start):               # the last round of the line holds no delimiter: one token fills it
            f = _File(ncols=3)
            s, a0 = start(f)
            f.add(b"r" * (a0 + ROUND - 40 - s), [b"5", b"7", b"0." + b"0" * 400 + b"25"])
            f.add(b"after")
            return f.data()

        def check_bare(d, smod=smod):
            s = d.index(b"\nr") + 1
            e = d.index(b"\n", s)
            a0 = s - smod
            assert e - a0 > ROUND and b"\t" not in d[a0 + ROUND:e] and b"\t" in d[a0 + ROUND - 64:a0 + ROUND]
        out.append(_case(f"last_round_without_delimiter_s{smod}", "rounds", bare_last_round, b"\t", 3, "device", check_bare))
    return out


def _tall(G, width=7):
    """G lines "g<width digits>\\t<digit>\\n" as one byte array, and the header."""
    rng = np.random.default_rng(G)
    a = np.empty((G, width + 4), np.uint8)
    a[:, 0] = ord("g")
    idx = np.arange(G)
    for k in range(width):
        a[:, width - k] = 48 + (idx // 10**k) % 10
    a[:, width + 1] = 9
    a[:, width + 2] = 48 + rng.integers(0, 10, G)
    a[:, width + 3] = 10
    return b"ID\tv\n", a


def _shape_cases():
    out = []

    def one_row():
        return b"ID\ta\tb\tc\nonly\t1\t2.5\t-3\n"
    out.append(_case("one_row", "shapes", one_row, b"\t", 3, "device", lambda d: _assert(d.count(b"\n") == 2)))

    def one_col():
        return b"ID,v\n" + b"".join(b"g%d,%d\n" % (i, i * i) for i in range(50))
    out.append(_case("one_column", "shapes", one_col, b",", 1, "device",
                     lambda d: _assert(all(ln.count(b",") == 1 for ln in d.split(b"\n")[:-1]) and d.count(b"\n") == 51)))

    def tall():
        h, a = _tall(300_001)
        return h + a.tobytes()
    out.append(_case("tall_300001_by_1", "shapes", tall, b"\t", 1, "device", lambda d: _assert(d.count(b"\n") == 300_002)))

    def taller():                                       # above 256 blocks of 64 KiB: tbl_scan_blocks carries into a second pass
        h, a = _tall(1_600_000)
        return np.concatenate([np.frombuffer(h, np.uint8), a.ravel()])
    out.append(_case("tall_1600000_by_1_over_256_blocks", "shapes", taller, b"\t", 1, "device",
                     lambda d: _assert(len(d) > 256 * BLOCK + BLOCK)))
    for n in (0, 1, 15, 16, 17, 5000):
        def labels(n=n):
            f = _File(ncols=2)
            f.add(b"plain", [b"1", b"2"])
            f.add(b"Lab-el.of_some/length+more"[:n] if n < 20 else b"k" * n, [b"3", b"4.5"])
            f.add(b"other", [b"5", b"6"])
            return f.data()
        out.append(_case(f"label_of_{n}", "shapes", labels, b"\t", 2, "device",
                         lambda d, n=n: _assert(n in [len(x.split(b"\t")[0]) for x in d.split(b"\n")[1:-1]])))

    def odd_labels():
        f = _File(ncols=2, sep=b",", header=b"ID,a,b\n")
        for lab in (b"  spaced", b"two words", b"\xc3\xa9t\xc3\xa9", b"\xe6\x97\xa5\xe6\x9c\xac", b"del\x7fete", b"7SK", b"g-1.x", b"tab less"):
            f.add(lab, [b"1", b"0.25"])
        return f.data()
    out.append(_case("labels_spaces_utf8_del", "shapes", odd_labels, b",", 2, "device", lambda d: _assert(b"\x7f" in d and b"\xc3\xa9" in d)))
    for sep, name in ((b"\t", "tab"), (b",", "comma")):
        def crlf(sep=sep):
            rng = np.random.default_rng(len(sep) + 11)
            f = _File(ncols=4, sep=sep, eol=b"\r\n")
            for g in range(200):
                f.add(b"gene%d" % g, [b"%d" % rng.integers(0, 99), b"%.3f" % rng.normal(), b"0", b"%d" % rng.integers(0, 9)])
            return f.data()
        out.append(_case(f"crlf_throughout_{name}", "shapes", crlf, sep, 4, "device",
                         lambda d: _assert(d.count(b"\r\n") == 201 and d.count(b"\n") == 201)))
    return out


_ROW = 16384                                            # the chunk files' line length: CHUNK is a multiple of it


def _chunk_file(N, shift, crlf=False, final=True):
    """A file of exactly N bytes (the last byte a line end if `final`) whose data lines are _ROW bytes each, the first one starting at
    2 * _ROW + shift: the byte at in-line offset i of some line sits at the chunk edge minus one when i == (-1 - shift) mod _ROW.
    The last line's label takes up the remainder."""
    rng = np.random.default_rng(N % 1000 + shift % 97)
    eol = b"\r\n" if crlf else b"\n"
    C = (_ROW - 8) // 4                                 # "g<6 digits>" or "g<5 digits>" + C x "\t<3 digits>" + eol
    lab = 8 - len(eol)
    names = [b"c%d" % j for j in range(C)]
    H = 2 * _ROW + shift
    base = len(b"\t".join([b"ID"] + names) + eol)
    names[0] = b"c" * (H - base + 2)
    header = b"\t".join([b"ID"] + names) + eol
    assert len(header) == H
    body = N - H + (0 if final else len(eol))
    G = body // _ROW
    rest = body - G * _ROW
    a = np.empty((G, _ROW), np.uint8)
    a[:, 0] = ord("g")
    idx = np.arange(G)
    for k in range(lab - 1):
        a[:, lab - 1 - k] = 48 + (idx // 10**k) % 10
    v = a[:, lab:lab + 4 * C].reshape(G, C, 4)
    v[:, :, 0] = 9
    v[:, :, 1:] = 48 + rng.integers(0, 10, (G, C, 3), dtype=np.uint8)
    a[:, lab + 4 * C:] = np.frombuffer(eol, np.uint8)
    flat = a.ravel()
    if rest:                                            # lengthen the last line's label
        last = a[G - 1]
        flat = np.concatenate([a[:G - 1].ravel(), last[:1], np.full(rest, ord("p"), np.uint8), last[1:]])
    if not final:
        flat = flat[:len(flat) - len(eol)]
    out = np.concatenate([np.frombuffer(header, np.uint8), flat])
    assert len(out) == N
    return out, C


def _chunk_cases():
    out = []
    plan = [(1, -1, 0, False, True), (1, 0, 0, False, False), (1, 1, 0, False, True),
            (2, -1, 0, False, True),                    # a '\n' as the last byte of chunk 0
            (2, 0, 1, True, True),                      # '\r' the last byte of chunk 0, '\n' the first of chunk 1
            (2, 1, -9, False, False),                   # a token over the chunk edge
            (3, -1, -9, True, True), (3, 0, 1, True, False), (3, 1, 0, False, True)]
    for k, d, shift, crlf, final in plan:
        N = k * CHUNK + d
        C = (_ROW - 8) // 4

        def make(N=N, shift=shift, crlf=crlf, final=final):
            return _chunk_file(N, shift, crlf, final)[0]

        def check(a, N=N, k=k, shift=shift, crlf=crlf, final=final):
            assert len(a) == N and (a[-1] == 10) == final
            for m in range(1, k):
                E = m * CHUNK
                if shift == 0:
                    assert a[E - 1] == 10
                elif shift == 1:
                    assert a[E - 1] == 13 and a[E] == 10
                else:
                    assert 48 <= a[E - 1] <= 57 and 48 <= a[E] <= 57
        out.append(_case(f"chunks_{k}x{d:+d}_shift{shift}{'_crlf' if crlf else ''}{'' if final else '_open'}", "upload chunks", make,
                         b"\t", C, "device", check))
    return out


_INTS = [b"0", b"7", b"123456789012345", b"1234567890123456", b"9007199254740993", b"9999999999999999", b"-9007199254740993",
         b"999999999999999", b"9007199254740995", b"4503599627370497"]


def _check_integer_column(d):
    assert b"." not in d                                # no decimal token anywhere: every column is int64
    assert b"\t-0\n" in d or b"\t-0\t" in d
    assert b"\t12345678901234567\n" in d or b"\t12345678901234567\t" in d
    assert b"-123456789012345678\n" in d


def _distance_cases():
    """A float64 column whose only decimal token is far from its integer tokens: pandas reads the blocks between as int64 and casts."""
    out = []
    G = 300_000
    for where, name in ((0, "first"), (G // 2, "middle"), (G - 1, "last")):
        def tall(where=where):
            rng = np.random.default_rng(where + 1)
            pick = rng.integers(0, len(_INTS), G)
            lines = [b"g%d\t%s\t%d\n" % (g, _INTS[pick[g]], g % 10) for g in range(G)]
            lines[where] = b"g%d\t0.25\t3\n" % where
            lines[(where + G // 3) % G] = b"neg\t-0.0\t4\n"
            return b"ID\tx\ty\n" + b"".join(lines)
        out.append(_case(f"tall_decimal_in_{name}_line", "column types", tall, b"\t", 2, "device",
                         lambda d: _assert(d.count(b".") == 2 and d.count(b"\n") == G + 1)))
    W, R = 20_000, 40
    for where, name in ((0, "first"), (R // 2, "middle"), (R - 1, "last")):
        def wide(where=where):
            rng = np.random.default_rng(where + 100)
            pick = rng.integers(0, len(_INTS), (R, W))
            rows = [[_INTS[p] for p in pick[r]] for r in range(R)]
            for c in range(0, W, 3):                    # every third column is float64 through one decimal token
                rows[where][c] = b"0.25"
            rows[(where + 13) % R][0] = b"-0.0"
            return b"\t".join(b"c%d" % j for j in range(W)) + b"\n" + b"".join(b"g%d\t" % r + b"\t".join(rows[r]) + b"\n" for r in range(R))
        out.append(_case(f"wide_decimal_in_{name}_line", "column types", wide, b"\t", W, "device",
                         lambda d: _assert(d.count(b"\n") == R + 1 and d.count(b"0.25") >= W // 3)))

    def ints_tall():
        lines = [b"g%d\t%d\n" % (g, g) for g in range(G)]
        lines[5] = b"z\t-0\n"
        lines[G // 2] = b"s\t12345678901234567\n"
        lines[G - 2] = b"e\t-123456789012345678\n"
        return b"ID\tx\n" + b"".join(lines)
    out.append(_case("tall_integer_column_negzero_17_18_digits", "column types", ints_tall, b"\t", 1, "device", _check_integer_column))

    def ints_wide():
        rows = [[b"1"] * W for _ in range(R)]
        rows[0][0], rows[5][0], rows[R - 1][0] = b"-0", b"12345678901234567", b"999999999999999999"
        rows[3][W - 1], rows[R - 1][W - 1] = b"-00", b"-123456789012345678"
        return b"\t".join(b"c%d" % j for j in range(W)) + b"\n" + b"".join(b"g%d\t" % r + b"\t".join(rows[r]) + b"\n" for r in range(R))
    out.append(_case("wide_integer_column_negzero_17_18_digits", "column types", ints_wide, b"\t", W, "device", _check_integer_column))
    return out


MILLION = "million_tokens"


@functools.lru_cache(maxsize=1)
def million_table():
    """1 000 lines of the converter test's tokens (SPECIAL, EXTRA's short forms and the in-grammar ones of 1.2 million random
    tokens: above 10^6), the integer tokens in columns of their own so that every column is int64 or made of decimal tokens
    only.  Returns (bytes, C)."""
    toks = [t for t in SPECIAL + EXTRA[:4] + random_tokens(1_200_000) if in_grammar(t)]
    assert len(toks) >= 1_001_000
    G = 1000
    ints = [t for t in toks if is_integer_token(t)]
    decs = [t for t in toks if not is_integer_token(t)]
    ci, cd = len(ints) // G, len(decs) // G
    cols = [ints[c * G:(c + 1) * G] for c in range(ci)] + [decs[c * G:(c + 1) * G] for c in range(cd)]
    order = np.random.default_rng(5).permutation(len(cols))
    cols = [cols[i] for i in order]
    C = len(cols)
    head = "ID\t" + "\t".join(f"c{j}" for j in range(C)) + "\n"
    body = "".join(f"g{g}\t" + "\t".join(col[g] for col in cols) + "\n" for g in range(G))
    return (head + body).encode(), C


def _token_cases():
    out = []
    _c = {}

    def million():
        data, C = million_table()
        _c["C"] = C
        return data
    # (C is known once the tokens are drawn)
    out.append(_case(MILLION, "tokens", million, b"\t", None, "device",
                     lambda d: _assert(d.count(b"\n") == 1001 and d.count(b"\t") >= 1001 * 1000 and b"e-3" in d)))

    def extra():
        f = _File(ncols=2, header=b"ID\tdec\tint\n")
        ints = [b"007", b"-0", b"12345678901234567", b"999999999999999999", b"+5", b"0", b"1", b"2"]
        # (18 digits before the point, the most the grammar takes, under integer-looking neighbours in pandas' first attempt)
        for i, t in enumerate(EXTRA + ["999999999999999999.5", "-999999999999999999e1"]):
            f.add(b"t%d" % i, [t.encode(), ints[i]])
        return f.data()
    out.append(_case("extra_forms_and_4000_byte_tokens", "tokens", extra, b"\t", 2, "device", lambda d: _assert(b"0" * 3997 in d)))
    return out


def _random_cases(count=2000):
    out = []
    for i in range(count):
        def make(i=i):
            ints, decs = token_pool()
            rng = np.random.default_rng(10_000 + i)
            G, C = int(rng.integers(1, 41)), int(rng.integers(1, 41))
            sep = b"," if i % 2 else b"\t"
            eol = b"\r\n" if rng.random() < 0.3 else b"\n"
            names = [b"c%d" % j for j in range(C)]
            if C > 2 and rng.random() < 0.2:            # duplicate column names
                names[int(rng.integers(1, C))] = names[0]
            f = _File(sep=sep, eol=eol, ncols=C, header=sep.join(names if rng.random() < 0.25 else [b"ID"] + names) + eol)
            kind = rng.integers(0, 3, C)                # a column of integer tokens, of decimal tokens, or of both
            style = int(rng.integers(0, 4))
            for g in range(G):
                row = []
                for c in range(C):
                    if kind[c] == 0:
                        t = ints[int(rng.integers(0, len(ints)))]
                    elif kind[c] == 1 or rng.random() < 0.5 or (G == 1):
                        t = decs[int(rng.integers(0, len(decs)))]
                    else:
                        t = ints[int(rng.integers(0, len(ints)))]
                        while not _safe_in_float_column(t):
                            t = ints[int(rng.integers(0, len(ints)))]
                    row.append(t.encode())
                lab = (b"g%d" % g, b"%d" % (g * 3), b"GENE %d" % (g % 5), b"x" * int(rng.integers(1, 30)))[style]
                f.add(lab, row, eol if g < G - 1 or rng.random() < 0.8 else b"")
            return f.data()
        def check(d, i=i):                              # one delimiter and one kind of line end per file, 1 ... 40 lines and columns
            sep, other = (b",", b"\t") if i % 2 else (b"\t", b",")
            lines = d.split(b"\n")
            assert other not in d and d.count(b"\r") in (0, d.count(b"\n"), d.count(b"\n") + 1) and d.count(b"\r\n") in (0, d.count(b"\n"))
            assert 2 <= len(lines) - (lines[-1] == b"") <= 41 and 1 <= lines[1].count(sep) <= 40
        out.append(_case(f"random_{i}", "random tables", make, b"," if i % 2 else b"\t", None, "device", check))
    return out


# ---- outside the grammar -----------------------------------------------------------------------------------------------------

_RANGE_TOKEN = b"1e309"


def _plant(kind, place):
    """One defect of `kind` at `place`: "first" / "last" (line), an absolute byte offset (the defect's position is that byte), or
    "eof" (the defect's last byte is the file's last).  Returns (make, intended)."""
    C = 3
    f = _File(ncols=C)
    dec = [b"4", b"0.5", b"6"]
    ok = [b"4", b"5", b"6"] if kind == INT_CAST else dec     # (INT_CAST: the column's one decimal token is in line a0 / the last line)

    def bad_line(at):
        """Append the defective line so that the defect's position is `at` (None: wherever the line falls).  Returns (pos, eol)."""
        if kind in (BYTE, QUOTE, CR):
            c = {BYTE: b"\x01", QUOTE: b'"', CR: b"\r"}[kind]
            if at is not None:
                f.fill_to(at - 3)
            s = f.add(b"lab" + c + b"el", ok)
            return s + 3
        if kind == BLANK:
            if at is not None:
                f.fill_to(at)
            return f.add_raw(b"\n")
        if kind == FIELDS:
            if at is not None:
                f.fill_to(at)
            return f.add(b"short", ok[:2])
        if kind in (TOKEN, RANGE, INT_CAST):
            t = {TOKEN: b"NA", RANGE: _RANGE_TOKEN, INT_CAST: b"12345678901234567"}[kind]
            if at is not None:
                f.fill_to(at - (6 if kind == INT_CAST else 4))
            s = f.add(b"lab", [b"4", t, b"6"] if kind == INT_CAST else [t, b"0.5", b"6"])
            if kind == INT_CAST and at is not None:
                assert s - f.starts[0] > 60_000                 # far from the decimal token: other blocks, a thousand lines between
            return s + (6 if kind == INT_CAST else 4)
    if place != "first":
        f.add(b"a0", dec)
    if place == "first":
        pos = bad_line(None)
        line = f.line_no()
        for g in range(4):
            f.add(b"t%d" % g, ok)
        f.add(b"dec", dec)
    elif place == "last":
        for g in range(4):
            f.add(b"t%d" % g, ok)
        pos = bad_line(None)
        line = f.line_no()
    elif place == "eof":
        for g in range(3):
            f.add(b"t%d" % g, ok)
        if kind in (BYTE, QUOTE, CR):
            c = {BYTE: b"\x1f", QUOTE: b'"', CR: b"\r"}[kind]
            f.add_raw(b"lab\t4\t0.5\t6" + c)
            pos = f.pos - 1
        elif kind == BLANK:
            pos = f.add_raw(b"\n")
        elif kind == FIELDS:
            pos = f.add_raw(b"x")
        elif kind == TOKEN:
            f.add_raw(b"lab\t4\t0.5\tx")
            pos = f.pos - 1
        elif kind == RANGE:
            f.add_raw(b"lab\t4\t0.5\t" + _RANGE_TOKEN)
            pos = f.pos - len(_RANGE_TOKEN)
        else:
            f.add_raw(b"lab\t4\t-0\t6")                # (INT_CAST names a column, not a byte)
            pos = 0
        line = f.line_no()
    else:
        pos = bad_line(int(place))
        assert pos == place, (pos, place)
        line = f.line_no()
        f.fill_to(f.pos + 200)
    data = f.data()
    if kind == INT_CAST:
        return data, (INT_CAST, 0, 1)
    return data, (kind, line, pos)


_KIND_NAME = {BYTE: "byte", QUOTE: "quote", CR: "cr", BLANK: "blank", FIELDS: "fields", TOKEN: "token", RANGE: "range", INT_CAST: "intcast"}
_PLACES = ["first", "last", "eof", BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK, 3 * BLOCK - 1, 3 * BLOCK, BLOCK + 37 * SPAN - 1, BLOCK + 37 * SPAN,
           BLOCK - SPAN - 1, BLOCK - SPAN, 2 * BLOCK + 16 * 1000 - 1, 2 * BLOCK + 16 * 1000]


def _refusal_cases():
    out = []
    for kind in range(2, 10):
        for place in _PLACES:
            data, intended = _plant(kind, place)        # (built twice: once for the triple, once per make(); tiny or ~200 KB)

            def make(kind=kind, place=place):
                return _plant(kind, place)[0]

            def check(d, kind=kind, place=place, intended=intended):
                if kind == INT_CAST:
                    return
                p = intended[2]
                if isinstance(place, int):
                    assert p == place
                if place == "eof":
                    assert p == len(d) - (len(_RANGE_TOKEN) if kind == RANGE else 1)
                want = {BYTE: None, QUOTE: b'"', CR: b"\r", BLANK: b"\n", FIELDS: None, TOKEN: None, RANGE: b"1"}[kind]
                if want:
                    assert d[p:p + 1] == want
                if kind in (BLANK, FIELDS):
                    assert d[p - 1:p] == b"\n"
                assert d[:p].count(b"\n") + 1 == intended[1]
            out.append(_case(f"{_KIND_NAME[kind]}_{place}", "one defect", make, b"\t", 3, intended, check))
            del data
    return out


def _two_defect_cases():
    out = []
    ok = [b"4", b"0.5", b"6"]

    def add(name, build):
        def make():
            return build()[0]
        out.append(_case(name, "two defects", make, b"\t", 3, build()[1]))

    def same_pass_blocks(c1, c2, k):
        def build():
            f = _File()
            f.fill_to(BLOCK - 10 - 3)
            s = f.add(b"lab" + c1 + b"el", ok)                     # the defect is byte BLOCK - 10: block 0
            line = f.line_no()
            f.fill_to(BLOCK + 30 - 3)
            f.add(b"lab" + c2 + b"el", ok)                         # the second one is byte BLOCK + 30: block 1
            f.fill_to(3 * BLOCK + 5)
            f.add(b"la" + c2 + b"b", ok)
            assert s + 3 == BLOCK - 10
            return f.data(), (k, line, BLOCK - 10)
        return build
    add("quote_in_block_0_and_1", same_pass_blocks(b'"', b'"', QUOTE))
    add("byte_in_block_0_quote_in_block_1", same_pass_blocks(b"\x02", b'"', BYTE))
    add("cr_in_block_0_byte_in_block_1", same_pass_blocks(b"\r", b"\x03", CR))

    def tokens_two_lines():
        f = _File()
        f.add(b"a", ok)
        s = f.add(b"b", [b"4", b"x5", b"6"])
        line = f.line_no()
        f.add(b"c", [b"NA", b"0.5", b"6"])
        return f.data(), (TOKEN, line, s + 4)
    add("bad_tokens_in_two_lines", tokens_two_lines)

    def tokens_two_blocks():
        f = _File()
        f.fill_to(BLOCK - 20)
        s = f.add(b"b", [b"4", b"0.5", _RANGE_TOKEN])
        line = f.line_no()
        f.fill_to(BLOCK + 100)
        f.add(b"c", [b"NA", b"0.5", b"6"])
        f.fill_to(2 * BLOCK + 50)
        f.add_raw(b"\n")
        f.add(b"d", ok)
        return f.data(), (RANGE, line, s + 8)
    add("range_in_block_0_token_in_block_1_blank_in_block_2", tokens_two_blocks)

    def blank_then_fields():
        f = _File()
        f.add(b"a", ok)
        s = f.add(b"short", ok[:1])
        line = f.line_no()
        f.add_raw(b"\n")
        return f.data(), (FIELDS, line, s)
    add("short_line_then_blank_line", blank_then_fields)

    def quote_far_behind():
        f = _File()
        f.add(b"a", [b"NA", b"0.5", b"6"])                          # a field-pass defect in the first line
        f.fill_to(2 * BLOCK + 1000)
        s = f.add(b'la"b', ok)
        line = f.line_no()
        f.add(b"z", ok)
        return f.data(), (QUOTE, line, s + 2)
    add("bad_token_early_quote_two_blocks_later", quote_far_behind)

    def blank_early_cr_late():
        f = _File()
        f.add(b"a", ok)
        f.add_raw(b"\n")
        for g in range(5):
            f.add(b"g%d" % g, ok)
        s = f.add(b"la\rb", ok)
        return f.data(), (CR, f.line_no(), s + 2)
    add("blank_line_early_lone_cr_later", blank_early_cr_late)

    def token_in_short_line():
        f = _File()
        f.add(b"a", ok)
        s = f.add(b"b", [b"NA", b"6"])
        line = f.line_no()
        f.add(b"c", ok)
        return f.data(), (FIELDS, line, s)
    add("bad_token_in_a_line_with_too_few_fields", token_in_short_line)

    def token_in_long_line():
        f = _File()
        f.add(b"a", ok)
        s = f.add(b"b", [b"NA", b"0.5", b"6", b"7"])
        line = f.line_no()
        return f.data(), (FIELDS, line, s)
    add("bad_token_in_a_line_with_too_many_fields", token_in_long_line)

    def token_beyond_c():
        f = _File()
        f.add(b"a", ok)
        s = f.add(b"b", ok + [b"NA", b"1e999"])
        line = f.line_no()
        f.add(b"c", ok)
        return f.data(), (FIELDS, line, s)
    add("bad_tokens_beyond_the_last_column", token_beyond_c)

    def cast_two_columns():
        f = _File()
        f.add(b"a", [b"1", b"-0", b"12345678901234567"])
        f.add(b"b", [b"2", b"0.5", b"1.5"])
        return f.data(), (INT_CAST, 0, 1)
    add("int_cast_in_two_columns", cast_two_columns)

    def cast_high_column_first_in_file():
        f = _File()
        f.add(b"a", [b"1", b"7", b"123456789012345678"])
        f.add(b"b", [b"0.5", b"0.5", b"1.5"])
        f.add(b"c", [b"-0", b"-00", b"3"])
        return f.data(), (INT_CAST, 0, 0)
    add("int_cast_lower_column_later_in_file", cast_high_column_first_in_file)

    def cast_and_token():
        f = _File()
        f.add(b"a", [b"1", b"-0", b"3"])
        f.add(b"b", [b"2", b"0.5", b"1.5"])
        f.fill_to(BLOCK + 300)
        s = f.add(b"c", [b"2", b"0.5", b"1.5.5"])
        return f.data(), (TOKEN, f.line_no(), s + 8)
    add("int_cast_and_a_bad_token_far_behind", cast_and_token)

    def cast_and_fields():
        f = _File()
        f.add(b"a", [b"1", b"-0", b"3"])
        f.add(b"b", [b"2", b"0.5", b"1.5"])
        s = f.add_raw(b"lonely")
        return f.data(), (FIELDS, f.line_no(), s)
    add("int_cast_and_a_short_last_line", cast_and_fields)

    def lone_cr_eof():
        f = _File()
        f.add(b"a", ok)
        f.add_raw(b"b\t4\t0.5\t6\r")
        return f.data(), (CR, f.line_no(), f.pos - 1)
    add("lone_cr_ends_the_file", lone_cr_eof)

    def cr_block_end_no_nl():
        f = _File()
        f.fill_to(BLOCK - 1 - 3)
        s = f.add(b"lab\rx", ok)                                    # '\r' is the last byte of block 0; '\n' only two bytes on
        line = f.line_no()
        f.add(b"z", ok)
        assert s + 3 == BLOCK - 1
        return f.data(), (CR, line, BLOCK - 1)
    add("cr_ends_block_newline_two_bytes_later", cr_block_end_no_nl)

    def cr_cr_nl():
        f = _File(eol=b"\r\n")
        f.fill_to(BLOCK - 1 - 9)
        s = f.add_raw(b"q\t4\t0.5\t6\r\r\n")                       # "\r\r\n": the first '\r' (byte BLOCK - 1) is not before a '\n'
        line = f.line_no()
        f.add(b"z", ok)
        assert s + 9 == BLOCK - 1
        return f.data(), (CR, line, BLOCK - 1)
    add("cr_cr_nl_over_block_edge", cr_cr_nl)

    def only_cr_line():
        f = _File(eol=b"\r\n")
        f.add(b"a", ok)
        s = f.add_raw(b"\r\n")                                      # a line of one '\r' is an empty line
        line = f.line_no()
        f.add(b"z", ok)
        return f.data(), (BLANK, line, s)
    add("line_of_one_cr", only_cr_line)
    return out


def _long_integer_part_cases():
    """A decimal token with more than 18 digits before the point: pandas' type for its column depends on the tokens above it."""
    out = []
    for name, above, tok in (("20_digits_below_an_integer", b"7", b"56963997270084518163.5"), ("uint64_overflow_first", None, b"18446744073709551616e0"),
                             ("19_digits_below_a_decimal", b"0.5", b"1234567890123456789.5"), ("negative_20_digits", b"1", b"-56963997270084518163.25")):
        def build(above=above, tok=tok):
            f = _File()
            if above is not None:
                f.add(b"a", [b"1", above, b"2"])
            s = f.add(b"b", [b"3", tok, b"4"])
            line = f.line_no()
            f.add(b"c", [b"5", b"0.25", b"6"])
            return f.data(), (TOKEN, line, s + 4)
        out.append(_case(f"token_{name}", "one defect", lambda build=build: build()[0], b"\t", 3, build()[1],
                         lambda d, build=build, tok=tok: _assert(d[build()[1][2]:].startswith(tok))))
    return out


def _host_check_cases():
    def header_only():
        return b"ID\ta\tb\tc\n"
    return [_case("no_data_lines", "host checks", header_only, b"\t", 3, (BLANK, 2, 9), lambda d: _assert(header_end(d) == len(d) == 9))]


# ---- the list ----------------------------------------------------------------------------------------------------------------

def cases(random_tables=2000):
    """Every case, in a fixed order.  A case's file is made when its make() is called, not here."""
    block_edges = [m * BLOCK + d for m in (1, 2, 3) for d in (-1, 0, 1)]
    span_edges = [BLOCK + 37 * SPAN + d for d in (-1, 0, 1)]
    out = _edge_cases("block edges", block_edges) + _edge_cases("thread spans", span_edges)
    out += _long_lines() + _slice_cases() + _round_cases() + _shape_cases() + _chunk_cases() + _distance_cases() + _token_cases()
    out += _random_cases(random_tables)
    out += _host_check_cases() + _refusal_cases() + _long_integer_part_cases() + _two_defect_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def ncols_of(case, data):
    """The case's ncols; for the cases that leave it open, what _table_on_device counts: the delimiters of the first data line."""
    if case.ncols is not None:
        return case.ncols
    d0 = header_end(data)
    first = bytes(data[d0:d0 + (1 << 22)]).split(b"\n")[0]
    return first.count(case.sep)


def is_large(case):
    return case.family == "upload chunks" or "over_256_blocks" in case.name


if __name__ == "__main__":
    count = collections.Counter(c.family for c in cases())
    for fam, n in count.items():
        print(f"{n:6d}  {fam}")
    print(f"{sum(count.values()):6d}  in all")
