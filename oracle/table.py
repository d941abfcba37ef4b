"""A plain model of cyto_table_read + cyto_table_fetch (csrc/table.hip), CPU only: test infrastructure, like oracle/jv.py.

table_model(data, sep, data_offset, ncols) says what the device reader returns for a file with those bytes, from DESIGN.md 4.1c and
include/cytohip.h: the data region is split on '\\n', one '\\r' is stripped, the line is split on sep.  Nothing here knows of the
kernels' blocks, slices, rounds or scans.  The token converter is not restated: kinds and values come from the host compilation of
parse_token (cyto_table_parse_tokens), which tests/test_read_table_cpu.py pins to pandas.

Two writings of the same rule: `_lines_plain` walks the lines in Python, `_lines_numpy` finds the same bounds with array searches
for files of millions of tokens; table_model picks by size and tests/test_read_table_model_cpu.py holds the two together."""
import ctypes

import numpy as np

BYTE, QUOTE, CR, BLANK, FIELDS, TOKEN, RANGE, INT_CAST = 2, 3, 4, 5, 6, 7, 8, 9         # CYTO_TABLE_ERR_* (include/cytohip.h)
KIND_NAMES = {BYTE: "control byte", QUOTE: "quote", CR: "carriage return", BLANK: "blank line", FIELDS: "field count",
              TOKEN: "token", RANGE: "out of range", INT_CAST: "integer cast in a float column"}
_TOK_INT, _TOK_DEC, _TOK_BAD, _TOK_RANGE = 0, 1, 2, 3


def parse_spans(buf, starts, stops):
    """The host converter on the tokens buf[starts[i]:stops[i]] of one byte buffer (a uint8 array or a memory map; the spans in
    file order).  Returns (kind, value, ints) as common.parse_table_tokens does.  The hook takes consecutive spans, so the gaps
    between the tokens go in as spans of their own and their results are dropped."""
    from cytospace_amd import _lib
    n = len(starts)
    off = np.empty(2 * n, np.int64)
    off[0::2], off[1::2] = starts, stops
    assert n == 0 or (np.diff(off) >= 0).all()
    m = max(2 * n - 1, 0)
    kind, value, ints = np.zeros(m, np.int8), np.zeros(m, np.float64), np.zeros(m, np.int64)
    if n:
        _lib.check(_lib.lib().cyto_table_parse_tokens(buf.ctypes.data, m, off.ctypes.data, value.ctypes.data, ints.ctypes.data,
                                                      kind.ctypes.data))
    return kind[0::2], value[0::2], ints[0::2]


def _lines_plain(data, sep, d0, C):
    """(s, e, nsep, label end, token starts, token stops) per data line, the obvious way."""
    N = len(data)
    body = data[d0:]
    parts = body.split(b"\n")
    if body.endswith(b"\n"):
        parts.pop()                                     # (a last line without its '\n' ends at N)
    S, E, nsep, lab, t0, t1 = [], [], [], [], [], []
    s = d0
    for raw in parts:
        line = raw[:-1] if raw.endswith(b"\r") else raw
        e = s + len(line)
        fields = line.split(sep)
        S.append(s), E.append(e), nsep.append(len(fields) - 1), lab.append(s + len(fields[0]))
        q = s + len(fields[0]) + 1
        for k, f in enumerate(fields[1:]):
            if k < C:                                   # only the first C tokens of a line are looked at
                t0.append(q), t1.append(q + len(f))
            q += len(f) + 1
        s += len(raw) + 1
    assert s == N + (0 if body.endswith(b"\n") else 1)
    a = lambda x: np.asarray(x, np.int64)               # noqa: E731
    return a(S), a(E), a(nsep), a(lab), a(t0), a(t1)


def _lines_numpy(buf, sep, d0, C):
    """The same six arrays by array searches: every '\\n' ends a line, every delimiter belongs to the line whose end follows it."""
    N = len(buf)
    region = buf[d0:]
    nl = np.flatnonzero(region == 10).astype(np.int64) + d0
    ends = nl if buf[N - 1] == 10 else np.append(nl, N)
    S = np.concatenate([[d0], ends[:-1] + 1]).astype(np.int64)
    E = ends - ((ends > S) & (buf[np.maximum(ends - 1, 0)] == 13))
    P = np.flatnonzero(region == sep[0]).astype(np.int64) + d0
    line = np.searchsorted(ends, P, side="left")
    nsep = np.bincount(line, minlength=len(ends)).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(nsep)[:-1]])
    rank = np.arange(len(P)) - first[line]
    lab = E.copy()
    lab[nsep > 0] = P[first[nsep > 0]]
    nxt = np.append(P[1:], N)
    last_of_line = np.append(line[1:] != line[:-1], True)
    stop = np.where(last_of_line, E[line], nxt)
    keep = rank < C
    return S, E, nsep, lab, P[keep] + 1, stop[keep]


def table_model(data, sep, data_offset, ncols, vectorised=None, stats=False):
    """What cyto_table_read(path, sep, data_offset, ncols) and cyto_table_fetch return for a file holding `data` (bytes, or a uint8
    array / memory map for a large file).  sep: b"," or b"\\t".

    Accepted: {"status": 0, "G", "C", "values" (G x C int64 words; a float64 column's words are its values' bits), "is_float"
    (C int8), "labels" (uint8: label, sep, '\\n' per line)}; with stats also "two_step" and "subnormal", token counts for the
    converter test.
    Refused: {"status": 7, "reason": (kind, line, byte)}.  `line` is 1-based with the header as line 1: the data line holding
    `byte` is line 2 + the number of line ends ('\\n', and the end of file for a last line without one) below `byte`.

    Which refusal is reported, as the code has it:
      1. the host checks first: data_offset >= N is (BLANK, 2, N);
      2. the byte pass over [data_offset, N): the lowest position holding a '"' (QUOTE), a '\\r' not followed by '\\n' inside the
         file (CR), or a byte below 0x20 other than sep, '\\r', '\\n' (BYTE).  If there is one it wins over anything the field
         pass would find, wherever that is;
      3. the field pass: the lowest (position, kind) among an empty line (BLANK, at the line's first byte; a line of one '\\r' is
         empty), a line whose delimiter count is not C (FIELDS, at the line's first byte) and, for the first C tokens of a line
         only, a token outside the grammar (TOKEN) or out of range (RANGE), at the token's first byte;
      4. then the lowest column that holds both a decimal token and an integer token of 17 or 18 digits or a negative zero
         (INT_CAST, line 0, byte = the column)."""
    C = int(ncols)
    d0 = int(data_offset)
    N = len(data)
    big = N > (1 << 20) if vectorised is None else vectorised
    buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data
    sep = bytes(sep)
    assert sep in (b",", b"\t") and C > 0 and d0 >= 0

    def refused(kind, pos, ends=None):
        line = 0 if ends is None else 2 + int(np.searchsorted(ends, pos, side="left"))
        return {"status": 7, "reason": (kind, line, int(pos))}
    if d0 >= N:
        return {"status": 7, "reason": (BLANK, 2, N)}
    # (2) the byte pass; in slabs, so that a file of gigabytes needs no mask of its own size
    bad = None
    nl_parts = []
    for lo in range(d0, N, 1 << 26):
        r = buf[lo:min(N, lo + (1 << 26))]
        nl_parts.append(np.flatnonzero(r == 10).astype(np.int64) + lo)
        if bad is None:
            hit = np.flatnonzero((r == 34) | (r == 13) | ((r < 0x20) & (r != sep[0]) & (r != 10))).astype(np.int64) + lo
            crlf = (buf[hit] == 13) & (hit + 1 < N) & (buf[np.minimum(hit + 1, N - 1)] == 10)
            hit = hit[~crlf]
            if hit.size:
                c = int(buf[hit[0]])
                bad = (QUOTE if c == 34 else CR if c == 13 else BYTE, int(hit[0]))
    ends = np.concatenate(nl_parts)
    if buf[N - 1] != 10:
        ends = np.append(ends, N)
    if bad:
        return refused(bad[0], bad[1], ends)
    # (3) the field pass
    if big:
        S, E, nsep, lab, t0, t1 = _lines_numpy(buf, sep, d0, C)
    else:
        S, E, nsep, lab, t0, t1 = _lines_plain(bytes(data), sep, d0, C)
    G = len(S)
    assert G == len(ends) and (E <= ends).all()
    kind, value, ints = parse_spans(buf, t0, t1)
    cand = [(int(s), BLANK) for s in S[E == S][:1]]
    cand += [(int(s), FIELDS) for s in S[(nsep != C) & (E > S)][:1]]
    cand += [(int(p), TOKEN) for p in t0[kind == _TOK_BAD][:1]]
    cand += [(int(p), RANGE) for p in t0[kind == _TOK_RANGE][:1]]
    if cand:
        pos, k = min(cand)
        return refused(k, pos, ends)
    # (4) column types
    assert len(kind) == G * C
    kind, value, ints = kind.reshape(G, C), value.reshape(G, C), ints.reshape(G, C)
    is_float = (kind == _TOK_DEC).any(axis=0)
    ndig = np.zeros(G * C, np.int64)
    isint = (kind == _TOK_INT).ravel()
    first = buf[np.minimum(t0, N - 1)]
    ndig[isint] = (t1 - t0 - ((first == 43) | (first == 45)))[isint]
    cast = (isint & ((ndig >= 17) | ((ints.ravel() == 0) & np.signbit(value.ravel())))).reshape(G, C).any(axis=0)
    both = np.flatnonzero(is_float & cast)
    if both.size:
        return {"status": 7, "reason": (INT_CAST, 0, int(both[0]))}
    words = np.where(is_float[None, :], value.view(np.int64), ints)
    sub = (kind == _TOK_DEC) & (value != 0) & (np.abs(value) < np.finfo(np.float64).tiny)
    labels = np.frombuffer(b"".join(bytes(buf[s:l]) + sep + b"\n" for s, l in zip(S.tolist(), lab.tolist())), np.uint8)
    out = {"status": 0, "G": G, "C": C, "values": np.ascontiguousarray(words), "is_float": is_float.astype(np.int8), "labels": labels}
    if stats:
        out.update(two_step=_two_step(buf, t0, t1, kind.ravel()), subnormal=int(sub.sum()))
    return out


def _two_step(buf, t0, t1, kind):
    """A lower bound of how many decimal tokens end with a decimal exponent below -308 (the converter's two divisions): counted
    from the text, not by the converter, and only among tokens of the plain form <digits>[.<digits>]e<exponent> of at most 64
    bytes, which is how the generator writes the small ones; others are not counted."""
    n = 0
    for a, b in zip(t0[kind == _TOK_DEC], t1[kind == _TOK_DEC]):
        if b - a > 64:
            continue
        t = bytes(buf[a:b]).lower().lstrip(b"+-")
        if b"e" not in t:
            continue
        m, x = t.split(b"e")
        ip, _, fp = m.partition(b".")
        kept = (ip + fp)[:17]
        exp = int(x) + max(len(ip) - 17, 0) - max(len(kept) - min(len(ip), 17), 0)
        n += -616 <= exp < -308
    return n


def read_device(path, sep, data_offset, ncols, device_id=0):
    """cyto_table_read + cyto_table_fetch as common._table_on_device calls them, in the model's form."""
    from cytospace_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    shape, why = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    st = L.cyto_table_read(str(path).encode(), bytes(sep), int(data_offset), int(ncols), device_id, ctypes.byref(h), shape, why, None)
    if st == 7:
        return {"status": 7, "reason": (why[0], why[1], why[2])}
    _lib.check(st)
    try:
        G, C, nlab = shape
        values, is_float, labels = np.empty((G, C), np.int64), np.empty(C, np.int8), np.empty(nlab, np.uint8)
        _lib.check(L.cyto_table_fetch(h, values.ctypes.data, is_float.ctypes.data, labels.ctypes.data, None))
    finally:
        L.cyto_table_free(h)
    return {"status": 0, "G": G, "C": C, "values": values, "is_float": is_float, "labels": labels}
