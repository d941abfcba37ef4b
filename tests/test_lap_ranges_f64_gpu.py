"""The float64 LAP (lap_f64.hip) where the narrowing of its warm start leaves float32's range, and the float64 entry of the float32 solve.

The float64 solve narrows the matrix to float32, runs the float32 wide solver on the image and starts the float64 chain from its prices.
test_lap_f64_classes_gpu.py runs it within a few binades of 1, test_lap_gpu.py once where EVERY entry overflows (1e300, n = 50).  Here
the classes types, neg, dup4, sub32few of _f64_classes.py are solved at c * 2^k (exact in float64), n = 65, 300, 1200:

    k = +-100   the image is a normal float32 matrix                                      f64_warm == 1
    k = -140    the image is subnormal and inexact                                        f64_warm == 1
    k = -900    the image is all zeros: the warm prices carry nothing                     f64_warm == 1
    k = 900     every entry overflows: CYTO_ERR_NONFINITE from the float32 solve -> cold  f64_warm == 0
    rng.random((300, 300)) * 2^129: about half of the entries overflow                    f64_warm == 0

The reference is jv_oracle(c * 2^k, float64, warm=True) on the scaled matrix, bit for bit, as test_lap_gpu.py::_check_warm compares:
rowsol, colsol, u, v, STAT_KEYS -- and the total within 1e-12 * sum|c_assigned| (1e-9 * max(1, |total|) means nothing at 2^-900).  That
restatement is itself pinned across the range, against scipy and against the base solve scaled, in test_lap_ranges_cpu.py.
mode = 1 (the cold chain) at k = +-900: the oracle of the scaled matrix, which is the base cold solve's indices and duals * 2^k exactly.
cyto_lap_f32_from_f64 (lapjv_hip on a float64 host matrix, narrowed on the device): at 2^+-100 the float32 solve of astype(float32);
an entry of 2^129 is refused like 1e300.

Time on an MI355X host, oracles included: 62 s for the file.  46 s of that are the eight cells of `types` at k = +-900 (n = 65: 2.2 and
4.8 s, n = 300: 6.0 s, n = 1200: 11.2 s, and the two cold chains at n = 300: 6.1 s): with nothing to start from the float64 chain is cut
at the row reduction's step budget, 2.2 million row scans in one workgroup whatever n is (test_lap_f64_classes_gpu.py has the same
cells at k = 0).  Every other test takes 1 s or less.
"""
import numpy as np
import pytest

from _f64_classes import make
from cytospace_amd.lap import lap_solve, lapjv_hip
from oracle.jv import jv_oracle, jv_oracle_wide
from test_lap_gpu import STAT_KEYS, WIDE_KEYS

pytestmark = pytest.mark.gpu

CLASSES = ("types", "neg", "dup4", "sub32few")
WARM = {-900: 1, -140: 1, -100: 1, 100: 1, 900: 0}


def _equals(g, o, c, tag):
    n = len(c)
    for key in ("rowsol", "colsol", "u", "v"):
        assert np.array_equal(g[key], o[key]), (tag, key)
    assert np.array_equal(np.sort(g["colsol"]), np.arange(n)) and np.array_equal(g["rowsol"][g["colsol"]], np.arange(n)), tag
    assert np.isfinite(g["u"]).all() and np.isfinite(g["v"]).all(), tag
    assert abs(g["total"] - o["total"]) <= 1e-12 * float(np.abs(c[np.arange(n), o["rowsol"]]).sum()), (tag, g["total"], o["total"])
    gd, od = g["info"].as_dict(), o["stats"].as_dict()
    for key in STAT_KEYS:
        assert gd[key] == od[key], (tag, key, gd[key], od[key])


@pytest.mark.parametrize("k", sorted(WARM))
@pytest.mark.parametrize("n", [65, 300, 1200])
@pytest.mark.parametrize("cls", CLASSES)
def test_warm_start_where_narrowing_leaves_float32(cls, n, k):
    c = make(cls, n) * 2.0 ** k
    assert np.isfinite(c).all() and np.array_equal(c / 2.0 ** k, make(cls, n))
    g = lap_solve(c, np.float64, return_info=True)
    assert g["info"].f64_warm == WARM[k], (cls, n, k)
    _equals(g, jv_oracle(c, np.float64, warm=True), c, (cls, n, k))


def test_warm_start_when_part_of_the_matrix_overflows():
    c = np.random.default_rng(129).random((300, 300)) * 2.0 ** 129
    with np.errstate(over="ignore"):
        over = np.isinf(c.astype(np.float32))
    assert 0.3 < over.mean() < 0.7                                  # FLT_MAX is just below 2^128: about half of U(0, 2^129)
    g = lap_solve(c, np.float64, return_info=True)
    assert g["info"].f64_warm == 0
    _equals(g, jv_oracle(c, np.float64, warm=True), c, "2^129")


@pytest.mark.parametrize("k", [-900, 900])
@pytest.mark.parametrize("cls", CLASSES)
def test_cold_chain_at_the_ends_of_the_double_range(cls, k):
    n = 300
    c0 = make(cls, n)
    c = c0 * 2.0 ** k
    g = lap_solve(c, np.float64, return_info=True, opts=dict(mode=1))
    assert g["info"].f64_warm == 0
    _equals(g, jv_oracle(c, np.float64), c, (cls, k))
    b = jv_oracle(c0, np.float64)
    assert np.array_equal(g["rowsol"], b["rowsol"]) and np.array_equal(g["colsol"], b["colsol"])
    assert np.array_equal(g["u"], b["u"] * 2.0 ** k) and np.array_equal(g["v"], b["v"] * 2.0 ** k)


@pytest.mark.parametrize("k", [-100, 100])
@pytest.mark.parametrize("n", [130, 300])
def test_float64_host_matrix_narrowed_on_the_device_at_both_scales(n, k):
    c64 = np.random.default_rng([n, 64]).random((n, n)) * 2.0 ** k
    c32 = c64.astype(np.float32)
    assert not np.array_equal(c32.astype(np.float64), c64) and 2.0 * n * float(np.abs(c32).max()) < 2.0 ** 127     # narrowing rounds
    row, col, (tot, u, v) = lapjv_hip(c64)
    ref = lap_solve(c32, np.float32, return_info=True)
    assert np.array_equal(row, ref["rowsol"]) and np.array_equal(col, ref["colsol"])
    assert np.array_equal(u, ref["u"]) and np.array_equal(v, ref["v"]) and tot == ref["total"]
    o = jv_oracle_wide(c32, np.float32)
    for key in ("rowsol", "colsol", "u", "v"):
        assert np.array_equal(ref[key], o[key]), key
    gd, od = ref["info"].as_dict(), o["stats"].as_dict()
    for kg, ko in WIDE_KEYS:
        assert gd[kg] == od[ko], (kg, gd[kg], od[ko])


def test_float64_host_matrix_beyond_float32_is_refused():
    c = np.random.default_rng(7).random((64, 64))
    c[40, 3] = 2.0 ** 129
    with pytest.raises(ValueError):
        lapjv_hip(c)
