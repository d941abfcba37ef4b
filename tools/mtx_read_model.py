"""A plain model of cyto_mtx_read (csrc/mtx_read.hip) and seeded MatrixMarket files that know their outcome.

mtx_model restates the body pass the plain way: the byte check, split on '\\n', strip one '\\r', the entry lines through the host
compilation of the kernel's parser (common.parse_mtx_entries), a numpy scatter.  cases() generates files inside the device grammar
(intended == "device") and files with one planted defect of every kind, or two, whose refusal (kind, line, byte) is known from
the construction.  tests/test_read_mtx_cpu.py holds the model to those outcomes and to read_file; tests/test_read_mtx_gpu.py holds
the kernels to read_file on files of the same generator."""
import collections

import numpy as np

KIND_NAMES = {1: "io", 2: "byte", 3: "carriage return", 4: "entry count", 5: "blank line", 6: "fields", 7: "index", 8: "token",
              9: "inexact", 10: "negative zero", 11: "duplicate entry", 12: "memory"}
ALLOWED = frozenset(b"0123456789-.eE+ \t\r\n")


def mtx_model(data, d0, G, C, nnz, field):
    """cyto_mtx_read on the file's bytes.  {"status": 0, "words": G x C int64 (float64 bits for field 1), "entries",
    "duplicates"} or {"status": 7, "reason": (kind name, line, byte)}."""
    from cytospace_amd.common import parse_mtx_entries
    head_lines = data[:d0].count(b"\n")
    body = data[d0:]

    def refuse(kind, line, byte):
        return {"status": 7, "reason": (KIND_NAMES[kind], int(line), int(byte))}

    def line_of(pos):
        return head_lines + data[d0:pos].count(b"\n") + 1
    for i, c in enumerate(body):
        if c not in ALLOWED or (c in b" \t" and d0 + i == len(data) - 1):       # (scipy 1.15 reads beyond a blank that ends the file)
            return refuse(2, line_of(d0 + i), d0 + i)
        if c == 13 and body[i + 1:i + 2] != b"\n":
            return refuse(3, line_of(d0 + i), d0 + i)
    lines = body.split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                       # (the piece behind the last '\n'; an empty body has no line at all)
    if len(lines) != nnz:
        return refuse(4, 0, len(lines))
    starts = d0 + np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])[:-1].astype(np.int64)
    lines = [x[:-1] if x.endswith(b"\r") else x for x in lines]
    kind, where, row, col, val = parse_mtx_entries(lines, field, G, C)
    bad = np.flatnonzero(kind)
    if len(bad):
        i = bad[0]
        return refuse(int(kind[i]), head_lines + i + 1, starts[i] + where[i])
    words = np.zeros((G, C), np.int64)
    cell = (row - 1) * C + (col - 1)
    live = np.flatnonzero(val != 0)                       # a zero leaves its cell alone
    if field == 1:
        seen = {}
        for i in live:
            if cell[i] in seen:
                return refuse(11, head_lines + i + 1, starts[i])
            seen[cell[i]] = i
        words.reshape(-1)[cell[live]] = val[live]
        dups = 0
    else:
        with np.errstate(over="ignore"):
            np.add.at(words.reshape(-1), cell[live], val[live])
        dups = len(live) - len(np.unique(cell[live]))     # (what the device counts when every value is positive)
    return {"status": 0, "words": words, "entries": nnz, "duplicates": dups}


# ---- value tokens

def real_tokens(rng, n):
    """n value tokens of a real file in the forms the grammar names, inside and around its window: up to 17 digits split by an
    optional point, trailing zeros, exponents to +-25, signs, and the hand-written edges."""
    out = list(EDGE_REAL)
    while len(out) < n:
        nd = int(rng.integers(1, 18))
        digits = "".join(map(str, rng.integers(0, 10, nd)))
        if rng.random() < 0.3:
            digits = digits[:max(1, nd - int(rng.integers(1, 6)))].ljust(nd, "0")
        form = rng.integers(0, 4)
        if form == 0:
            tok = digits
        else:
            k = int(rng.integers(0, nd + 1))
            tok = digits[:k] + "." + digits[k:]
        if rng.random() < 0.5:
            tok += "eE"[int(rng.integers(2))] + ["", "+", "-"][int(rng.integers(3))] + str(int(rng.integers(0, 26)))
        if rng.random() < 0.3:
            tok = "-" + tok
        out.append(tok)
    return out[:n]


EDGE_REAL = ["999999999999999", "1000000000000000", "9999999999999999", "99999999999999.9e22", "0.999999999999999", "1e22", "1e23",
             "1e-22", "1e-23", "1.5e23", "15e22", "123456789012345e22", "123456789012345e-22", "1.23456789012345e8", "1e+22", "1E-22",
             "5.", ".5", "5.0", "5.000", "0.5000", "100", "100.000e2", "0", "0.0", "0e5", "-0", "-0.0", "-0e0", "-.0", "-5", "-5.5e-3",
             "+5", "+5.5", "5e+", "5e", "e5", ".", "-", "-.", "5..5", "5.5.5", "1e12345", "1e1234", "1e0001", "--5", "5-", "5e5e5",
             "0.000000000000000000000001", "0.0000000000000000000001", "1000000000000000000000", "000000000000000000005",
             "0000000000000000000000.5"]
EDGE_INT = ["0", "-0", "5", "-5", "007", "999999999999999999", "-999999999999999999", "1000000000000000000", "+5", "5.", "5.5", "5e1",
            "-", "", "--5", "5-"]


def int_tokens(rng, n):
    out = [t for t in EDGE_INT if t]
    while len(out) < n:
        nd = int(rng.integers(1, 20))
        tok = "".join(map(str, rng.integers(0, 10, nd)))
        out.append(("-" if rng.random() < 0.3 else "") + tok)
    return out[:n]


# ---- files

Case = collections.namedtuple("Case", "name family field G C nnz data d0 intended")


def header(field, G, C, nnz, comment=b"%\n", eol=b"\n"):
    banner = b"%%MatrixMarket matrix coordinate " + (b"integer" if field == 0 else b"real") + b" general" + eol
    return banner + comment + b"%d %d %d" % (G, C, nnz) + eol


def label_files(G, C):
    """The gene and cell lists of a G x C file: {"genes.tsv": ..., "barcodes.tsv": ...}."""
    return {"genes.tsv": "".join(f"g{i}\n" for i in range(G)).encode(), "barcodes.tsv": "".join(f"c{j}\n" for j in range(C)).encode()}


def write_case(directory, case):
    """The case as a 10x directory; returns the path of its matrix.mtx."""
    import os
    os.makedirs(directory, exist_ok=True)
    for name, text in label_files(case.G, case.C).items():
        with open(os.path.join(directory, name), "wb") as f:
            f.write(text)
    p = os.path.join(directory, "matrix.mtx")
    with open(p, "wb") as f:
        f.write(case.data)
    return p


def _value(rng, field):
    if field == 0:
        return b"%d" % int(rng.integers(1, 1000)) if rng.random() < 0.9 else b"-%d" % int(rng.integers(0, 10 ** 17))
    return real_tokens(rng, len(EDGE_REAL) + 1)[-1].encode()      # (one random token; _real_window_ok rewrites what is refused)


def _entries(rng, field, G, C, nnz, style):
    """nnz entry lines (without line ends) at distinct cells, plus their cells.  style: "plain" single spaces; "blanks" tabs,
    runs of blanks, leading and trailing blanks, zero-padded indices."""
    cells = rng.choice(G * C, size=nnz, replace=False) if nnz else np.zeros(0, np.int64)
    lines = []
    for c in cells:
        r, k, v = b"%d" % (c // C + 1), b"%d" % (c % C + 1), _value(rng, field)
        if style == "plain":
            lines.append(r + b" " + k + b" " + v)
        else:
            gap = lambda lo: bytes(rng.choice(list(b" \t"), size=int(rng.integers(lo, 4))).tolist())
            if rng.random() < 0.2:
                r = b"0" * int(rng.integers(1, 3)) + r
            lines.append(gap(0) + r + gap(1) + k + gap(1) + v + gap(0))
    return lines, cells


def _join(lines, eol, final=True):
    return eol.join(lines) + (eol if final and lines else b"")


def _real_window_ok(lines):
    """Keeps a generated real file inside the window: entries whose value token the parser would refuse are rewritten as 1.5."""
    from cytospace_amd.common import parse_mtx_entries
    kind = parse_mtx_entries(lines, 1, 10 ** 18, 10 ** 18)[0]
    return [x if k == 0 else x.rstrip(b" \t").rsplit(None, 1)[0] + b" 1.5" for x, k in zip(lines, kind)]


def cases(seed=0):
    rng = np.random.default_rng(seed)
    out = []

    def add(name, family, field, G, C, head, lines, eol, final, intended, nnz=None):
        if not final and lines and intended == "device":
            lines = lines[:-1] + [lines[-1].rstrip(b" \t")]
        data = head + _join(lines, eol, final)
        out.append(Case(name, family, field, G, C, len(lines) if nnz is None else nnz, data, len(head), intended))

    def valid(field, G, C, nnz, style):
        lines, cells = _entries(rng, field, G, C, nnz, style)
        return (_real_window_ok(lines) if field == 1 else lines), cells

    # inside the grammar
    for k in range(40):
        field = k & 1
        G, C = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        nnz = int(rng.integers(0, G * C + 1))
        style = "plain" if k % 4 < 2 else "blanks"
        eol = b"\r\n" if k % 8 >= 4 else b"\n"
        comment = b"%" + b"x" * int(rng.integers(0, 300)) + eol if k % 3 else b""
        lines, _ = valid(field, G, C, nnz, style)
        add(f"ok{k}", "accepted", field, G, C, header(field, G, C, nnz, comment, eol), lines, eol, k % 5 != 0, "device")
    for field in (0, 1):
        add(f"empty{field}", "accepted", field, 3, 4, header(field, 3, 4, 0), [], b"\n", True, "device")
        add(f"corner{field}", "accepted", field, 5, 7, header(field, 5, 7, 4), [b"1 1 1", b"1 7 2", b"5 1 3", b"5 7 4"], b"\n", True,
            "device")
        add(f"zeros{field}", "accepted", field, 2, 2, header(field, 2, 2, 3), [b"1 1 0", b"1 1 7", b"1 1 0"], b"\n", True, "device")
    add("dupsum", "accepted", 0, 4, 4, header(0, 4, 4, 7),
        [b"2 2 5", b"1 1 1", b"1 1 2", b"3 3 1", b"3 3 1", b"3 3 1", b"2 2 6"], b"\n", True, "device")
    add("dupwrap", "accepted", 0, 1, 1, header(0, 1, 1, 12), [b"1 1 999999999999999999"] * 12, b"\n", True, "device")

    # one planted defect of every kind: (kind, the text that replaces or joins line i, where in that line the refusal points)
    # The refusal names line i + at (0-based in the body; the header has four lines) at offset `where` of that line.
    def planted(name, field, mutate, kind, where=0, nnz_delta=0, eol=b"\n", second=None, at=0):
        G, C = 9, 11
        lines, _ = valid(field, G, C, 30, "plain")
        i = int(rng.integers(1, 28))
        if second is not None:
            lines[i + 1] = second(lines[i + 1], lines[i])
        lines[i] = mutate(lines[i])
        head = header(field, G, C, 30 + nnz_delta, b"%one\n%two\n")
        start = len(head) + sum(len(x) + len(eol) for x in lines[:i + at])
        w = where(lines[i + at]) if callable(where) else where
        intended = (kind, 4 + i + at + 1, start + w) if kind != "entry count" else (kind, 0, len(lines))
        add(name, "refused", field, G, C, head, lines, eol, True, intended, nnz=30 + nnz_delta)

    third = lambda x: len(x.rsplit(b" ", 1)[0]) + 1       # offset of the value token
    second_tok = lambda x: x.index(b" ") + 1
    for field in (0, 1):
        f = f"{field}"
        planted("byte" + f, field, lambda x: x.replace(b" ", b",", 1), "byte", lambda x: x.index(b","))
        planted("percent" + f, field, lambda x: b"%c", "byte")
        planted("cr" + f, field, lambda x: x.replace(b" ", b"\r", 1), "carriage return", lambda x: x.index(b"\r"))
        planted("count_short" + f, field, lambda x: x, "entry count", nnz_delta=1)
        planted("count_long" + f, field, lambda x: x, "entry count", nnz_delta=-1)
        planted("blank" + f, field, lambda x: b"", "blank line")
        planted("blank_crlf" + f, field, lambda x: b"", "blank line", eol=b"\r\n")
        planted("two" + f, field, lambda x: x.rsplit(b" ", 1)[0], "fields")
        planted("four" + f, field, lambda x: x + b" 1", "fields")
        planted("onlyblanks" + f, field, lambda x: b" \t ", "fields")
        planted("row0" + f, field, lambda x: b"0 " + x.split(b" ", 1)[1], "index")
        planted("rowbig" + f, field, lambda x: b"10 " + x.split(b" ", 1)[1], "index")
        planted("colbig" + f, field, lambda x: x.split(b" ")[0] + b" 12 " + x.split(b" ")[2], "index", second_tok)
        planted("colneg" + f, field, lambda x: x.split(b" ")[0] + b" -1 " + x.split(b" ")[2], "index", second_tok)
        planted("row19" + f, field, lambda x: b"0000000000000000001 " + x.split(b" ", 1)[1], "index")
        planted("plus" + f, field, lambda x: x.rsplit(b" ", 1)[0] + b" +5", "token", third)
        planted("both" + f, field, lambda x: x.rsplit(b" ", 1)[0] + b" +5", "token", third, second=lambda nxt, x: b"")
        planted("lower_first" + f, field, lambda x: b"0 " + x.split(b" ", 1)[1], "index", second=lambda nxt, x: nxt + b" 9")
    G, C = 3, 3
    for field, last in ((0, b"3 3 7 "), (1, b"3 3 7.5\t")):
        head = header(field, G, C, 2)
        add(f"open_blank{field}", "refused", field, G, C, head, [b"1 1 5", last], b"\n", False,
            ("byte", 5, len(head) + 6 + len(last) - 1))
    planted("int_point", 0, lambda x: x.rsplit(b" ", 1)[0] + b" 5.5", "token", third)
    planted("int_exp", 0, lambda x: x.rsplit(b" ", 1)[0] + b" 5e1", "token", third)
    planted("int19", 0, lambda x: x.rsplit(b" ", 1)[0] + b" 1000000000000000000", "token", third)
    planted("real_2points", 1, lambda x: x.rsplit(b" ", 1)[0] + b" 5.5.5", "token", third)
    planted("real_16", 1, lambda x: x.rsplit(b" ", 1)[0] + b" 1234567890.123456", "inexact", third)
    planted("real_e23", 1, lambda x: x.rsplit(b" ", 1)[0] + b" 1e23", "inexact", third)
    planted("real_negzero", 1, lambda x: x.rsplit(b" ", 1)[0] + b" -0.0", "negative zero", third)
    # (two non-zero entries in one cell: the second one is named; a zero before or between them is none)
    planted("real_dup", 1, lambda x: x.rsplit(b" ", 1)[0] + b" 1.5", "duplicate entry", at=1,
            second=lambda nxt, x: x.rsplit(b" ", 1)[0] + b" 2.5")
    return out
