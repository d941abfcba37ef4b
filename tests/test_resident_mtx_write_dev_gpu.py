"""cyto_mtx_write_dev (csrc/mtx.hip) at the C ABI: the matrix lies on the device with the CALLER's pitch and base, which mtx_count and
mtx_format take as they come.  The reference is the bytes scipy.io.mmwrite writes for coo_matrix(x[:, cols]) at run time
(tests/_text_values.scipy_bytes); the file must be byte-identical.  Every element of the input buffer that is not data is a poison
(tests/_layouts.py: NaN for the real types, the type's maximum for the integer ones): read as data it is a non-zero entry of the file
(or, as a NaN, a refusal), so the equality of the bytes covers the padding.  The one shape scipy treats differently -- a square
result, which it searches for symmetry -- is refused as the header documents (CYTO_MTX_ERR_SQUARE, nothing left at the path)."""
import ctypes
import os

import numpy as np
import pytest

import _layouts as LY
from _text_values import CODES, FRACTIONS, UNSUPPORTED, mixed_matrix, scipy_bytes
from cytospace_amd import _lib

pytestmark = pytest.mark.gpu

GS, NS = (1, 33, 300), (1, 130)
SMALL_BLOCK = 200                      # bytes: at G = 300 even a single column's body (a line per non-zero) is cut at least three times
REAL_LAYOUTS = ("tight", "odd_pitch", "offset_base")


def column_lists(N):
    return {"identity": np.arange(N, dtype=np.int64),
            "reversed with repeats": np.ascontiguousarray(np.r_[np.arange(N)[::-1], 0, N - 1, 0].astype(np.int64)),
            "single": np.array([N - 1], np.int64)}                   # (the column next to the pitch padding)


def integer_matrix(dtype, G, N, seed):
    """Counts with a zero in every other place and, here and there, the large values of the type below its maximum (the poison)."""
    rng = np.random.default_rng(seed)
    x = rng.poisson(0.8, (G, N)).astype(np.int64)
    top = np.iinfo(dtype).max - 1
    big = rng.random((G, N)) < 0.1
    x[big] = rng.integers(1000, top, int(big.sum()), endpoint=True)
    if np.dtype(dtype).kind == "i":
        x[rng.random((G, N)) < 0.1] *= -1
    x = x.astype(dtype)
    x.flat[0] = 7                                                  # (the first and the last element are entries)
    x.flat[-1] = top
    return np.ascontiguousarray(x)


def write_dev(path, dev_ptr, G, N, ld, code, cols, block_bytes, flags):
    with open(path, "wb") as f:
        f.write(b"stale, and longer than the matrix" * 100)
    info = _lib.MtxInfo()
    info.ms_upload = -1.0
    st = _lib.lib().cyto_mtx_write_dev(path.encode(), G, N, dev_ptr, ld, code, cols.ctypes.data, len(cols), block_bytes, 0, flags,
                                       ctypes.byref(info))
    return st, info


def run_layout(tmp_path, dtype, layout, make, flags):
    path = str(tmp_path / "m.mtx")
    fails, squares, cut = [], 0, 0
    for G in GS:
        for N in NS:
            x = make(dtype, G, N, 1000 * G + N)
            host, lead, ld = LY.build(x, layout, 4, np.nan)
            buf = _lib.DeviceBuffer.from_numpy(host)
            try:
                for name, cols in column_lists(N).items():
                    tag = f"{np.dtype(dtype).name} {layout} G={G} N={N} ld={ld} {name}"
                    for cap in (0, SMALL_BLOCK):
                        st, info = write_dev(path, buf.ptr + lead * host.itemsize, G, N, ld, CODES[np.dtype(dtype)], cols, cap, flags)
                        if G == len(cols):
                            squares += 1
                            if st != UNSUPPORTED or info.reason != _lib.CYTO_MTX_ERR_SQUARE or os.path.exists(path):
                                fails.append(f"{tag}: a square result must be refused (status {st}, reason {info.reason})")
                            continue
                        if st != 0:
                            fails.append(f"{tag} cap {cap}: status {st}, reason {info.reason}")
                            continue
                        want = scipy_bytes(x, cols)
                        got = open(path, "rb").read()
                        nnz = int(want.split(b"\n")[2].split()[2])
                        if got != want:
                            fails.append(f"{tag} cap {cap}: the file differs from scipy's ({len(got)} bytes, scipy {len(want)}; "
                                         f"nnz {info.nnz}, scipy {nnz})")
                        if info.nnz != nnz or info.bytes != len(want):
                            fails.append(f"{tag} cap {cap}: info.nnz {info.nnz} / bytes {info.bytes}, scipy {nnz} / {len(want)}")
                        if not info.ms_upload > 0.0:
                            fails.append(f"{tag} cap {cap}: ms_upload {info.ms_upload} is not reported")
                        if G == 300 and cap:
                            cut += 1
                            if info.blocks < 3:
                                fails.append(f"{tag} cap {cap}: {info.blocks} blocks, at least three were meant")
                if not np.array_equal(buf.to_numpy(host.shape, host.dtype).view(np.uint8), host.view(np.uint8)):
                    fails.append(f"{np.dtype(dtype).name} {layout} G={G} N={N}: the caller's matrix changed")
            finally:
                buf.free()
    assert squares == 6 and cut == 6                                # (G = 1 with one column: three lists, two caps; G = 300: every list)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:20])


@pytest.mark.parametrize("layout", LY.LAYOUTS)
@pytest.mark.parametrize("dtype", [np.uint16, np.int64], ids=lambda d: np.dtype(d).name)
def test_integer_matrices_in_every_layout(dtype, layout, tmp_path):
    run_layout(tmp_path, dtype, layout, integer_matrix, 0)


@pytest.mark.parametrize("layout", REAL_LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_real_matrices_with_fractions(dtype, layout, tmp_path):
    run_layout(tmp_path, dtype, layout, lambda dt, G, N, seed: mixed_matrix(dt, G, N, seed, zeros=0.5), FRACTIONS)
