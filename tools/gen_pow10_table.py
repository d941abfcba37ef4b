"""Writes cytospace_amd/csrc/pow10_table.h: the 128-bit powers of ten of the shortest-digits routine (csrc/shortest.h).

Entry k - K_MIN, for K_MIN <= k <= K_MAX, is g(k) = ceil(10^k * 2^(127 - floor(log2(10^k)))): 10^k scaled so that its top bit is bit 127,
rounded up (exact for 0 <= k <= 55), as {high word, low word}.  Python integers only: no floating point is involved.

    python tools/gen_pow10_table.py            # rewrite the header
    python tools/gen_pow10_table.py --check    # exit 1 when the committed header differs
"""
import os
import sys

K_MIN, K_MAX = -292, 324          # -k of every float64: k = floor(log10(2^q)) or floor(log10(3/4 * 2^q)), q in [-1074, 971]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cytospace_amd", "csrc", "pow10_table.h")


def g(k):
    """ceil(10^k * 2^(127 - floor(log2(10^k)))) as an integer in [2^127, 2^128)."""
    if k >= 0:
        p = 10 ** k
        sh = p.bit_length() - 128                     # floor(log2 p) - 127
        v = p << -sh if sh <= 0 else -((-p) >> sh)    # (-((-p) >> sh): the ceiling of p / 2^sh)
    else:
        d = 10 ** -k
        # floor(log2(10^k)) = -bit_length(d) when d is no power of two (it never is for k < 0: d is a multiple of 5)
        sh = 127 + d.bit_length()
        v = -((-(1 << sh)) // d)
    assert (1 << 127) <= v < (1 << 128), k
    return v


def text():
    lines = ["// pow10_table.h -- written by tools/gen_pow10_table.py; do not edit.  {high, low} of ceil(10^k * 2^(127 - floor(log2(10^k)))),",
             "// k = %d .. %d (shortest.h reads entry k - POW10_MIN)." % (K_MIN, K_MAX)]
    for k in range(K_MIN, K_MAX + 1):
        v = g(k)
        lines.append("{0x%016Xull, 0x%016Xull},   // 10^%d" % (v >> 64, v & ((1 << 64) - 1), k))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    t = text()
    if "--check" in sys.argv:
        with open(OUT) as f:
            sys.exit(0 if f.read() == t else 1)
    with open(OUT, "w") as f:
        f.write(t)
