"""Where the bytes of a device-resident matrix lie: a pure-numpy builder of the layouts the C ABI accepts (include/cytohip.h,
"Device inputs"), with EVERY element of the buffer that is not data set to a poison value -- a kernel that reads one of them as
data, or steps rows by anything but `ld`, changes the answer.

    build(matrix, layout, W, poison) -> (buf, lead, ld)

buf is a 1-D host array of the matrix's dtype, `lead` the element offset of the matrix's base in it and `ld` the pitch in elements:
element (i, j) of the matrix is buf[lead + i * ld + j].  Uploaded into one device allocation (256-byte aligned, as hipMalloc's
are), the base is at `ptr + lead * itemsize`.  W is the width of the quads a kernel reads rows in: 4, or 2 for the float64 LAP rows.

    layout             pitch                                        base
    tight              ld = n                                       aligned
    padded             ld = round_up(n, W)                          aligned
    wide               ld = round_up(n, W) + 2 W                    aligned
    double             ld = round_up(2 n, W)                        aligned
    odd_pitch          the first ld > n that is no multiple of W    aligned
    offset_base        ld = round_up(n, W)                          one element in
    quad_offset_base   ld = round_up(n, W)                          one quad (W elements) in

One quad in is 16 bytes for float32 quads and for float64 pairs (still a 16-byte aligned base), 8 bytes for uint16 and 4 for uint8:
aligned for a quad of that type, not to 16 bytes.  TAIL poisoned elements follow the last row (the last row's own padding included:
the buffer always ends behind a full pitch).
"""
import numpy as np

LAYOUTS = ("tight", "padded", "wide", "double", "odd_pitch", "offset_base", "quad_offset_base")
POISONS = (-1e30, float("nan"), float("-inf"))
TAIL = 5
ALLOC_ALIGN = 256            # what the base of a device allocation is aligned to at least


def round_up(x, m):
    return -(-x // m) * m


def poison_value(dtype, poison):
    """The poison as an element of dtype: integer types take their maximum, whatever `poison` says."""
    dtype = np.dtype(dtype)
    if dtype.kind in "ui":
        return dtype.type(np.iinfo(dtype).max)
    return dtype.type(poison)


def pitch_and_lead(n, layout, W=4):
    """(ld, lead) of a matrix with rows of n elements in the named layout."""
    pad = round_up(n, W)
    if layout == "tight":
        return n, 0
    if layout == "padded":
        return pad, 0
    if layout == "wide":
        return pad + 2 * W, 0
    if layout == "double":
        return round_up(2 * n, W), 0
    if layout == "odd_pitch":
        return (n + 1 if (n + 1) % W else n + 2), 0
    if layout == "offset_base":
        return pad, 1
    if layout == "quad_offset_base":
        return pad, W
    raise ValueError(f"unknown layout {layout!r}")


def base_alignment(lead, itemsize):
    """The largest power of two (<= ALLOC_ALIGN) that divides the base's byte offset in the allocation."""
    off = lead * itemsize
    a = ALLOC_ALIGN
    while off % a:
        a //= 2
    return a


def data_mask(rows, n, lead, ld, skip_rows=()):
    """Boolean mask over the buffer: True where a matrix element lies (rows listed in skip_rows hold no data)."""
    m = np.zeros(lead + rows * ld + TAIL, bool)
    body = m[lead:lead + rows * ld].reshape(rows, ld)
    body[:, :n] = True
    if len(skip_rows):
        body[np.asarray(skip_rows), :] = False
    return m


def build(matrix, layout, W=4, poison=-1e30, skip_rows=()):
    """The matrix in the named layout; every other element -- and every element of the rows in skip_rows, which a row map never
    names -- is poison."""
    matrix = np.asarray(matrix)
    rows, n = matrix.shape
    ld, lead = pitch_and_lead(n, layout, W)
    buf = np.full(lead + rows * ld + TAIL, poison_value(matrix.dtype, poison), matrix.dtype)
    buf[lead:lead + rows * ld].reshape(rows, ld)[:, :n] = matrix
    if len(skip_rows):
        buf[lead:lead + rows * ld].reshape(rows, ld)[np.asarray(skip_rows), :] = poison_value(matrix.dtype, poison)
    return buf, lead, ld


def extract(buf, lead, ld, rows, n):
    """The rows x n block a buffer holds."""
    return buf[lead:lead + rows * ld].reshape(rows, ld)[:, :n]


def bits(a):
    """An array's bytes as unsigned words of its element size (NaN compares equal to itself, -0.0 differs from +0.0)."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
