"""cyto_downsample_dev (csrc/downsample.hip) at the C ABI: the matrices lie on the device with the CALLER's pitches and bases, which
ds_totals, ds_copy and ds_hist take as they come.  The reference is cytospace_amd.common.downsample (host numpy, the legacy global
RandomState) from the same seeded state:
  1. the G x C block of the output, bit for bit;
  2. key[624] and pos equal numpy's state after the reference run;
  3. words_out equals what the host form (cyto_downsample) reports for the same input (code against code; 2. is the primary check);
  4. every byte of the output buffer outside the block still holds the pattern it was filled with, and the input buffer -- whose
     every element that is not data is the type's maximum (tests/_layouts.py) -- is byte-identical afterwards.
Integer data and byte comparisons: nothing has a tolerance."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import _layouts as LY
from cytospace_amd import _lib
from cytospace_amd import common as gcommon

pytestmark = pytest.mark.gpu

TARGET = 150
FILL = 0xA5
IN = {"uint8": (np.uint8, _lib.CYTO_DTYPE_U8), "uint16": (np.uint16, _lib.CYTO_DTYPE_U16), "int32": (np.int32, _lib.CYTO_DTYPE_I32),
      "int64": (np.int64, _lib.CYTO_DTYPE_I64)}
OUT = {"int64": (np.int64, _lib.CYTO_DTYPE_I64), "uint16": (np.uint16, _lib.CYTO_DTYPE_U16)}
OUT_LAYOUTS = ("tight", "odd_pitch", "offset_base", "wide")
# every layout of x and every layout of out occurs (not the full product)
PAIRS = [(xl, OUT_LAYOUTS[i % len(OUT_LAYOUTS)]) for i, xl in enumerate(LY.LAYOUTS)]
U32P = ctypes.POINTER(ctypes.c_uint32)


def counts(G, C, seed, heavy=None, big=False):
    """G x C int64 counts below 256.  Cell c is heavy (151 ... 255 transcripts) where heavy[c], else light (0 ... 150); by default
    the even cells are heavy and the last one is light, so the first and the last cell are one of each.  A heavy cell always has a
    transcript in the last gene (G = 2049: gene 2048, the second chunk of ds_hist).  big: one heavy cell gets 70 000 transcripts
    more in one gene (a total beyond 16 bits; the wider input types only)."""
    rng = np.random.default_rng(seed)
    if heavy is None:
        heavy = np.arange(C) % 2 == 0
        heavy[C - 1] = C == 1
    x = np.zeros((G, C), np.int64)
    for c in range(C):
        T = int(rng.integers(TARGET + 1, 256)) if heavy[c] else int(rng.integers(0, TARGET + 1))
        if c == 2 and heavy[c]:
            T = TARGET + 1                                 # the smallest cell that is downsampled
        if c == 1 and not heavy[c]:
            T = TARGET                                     # the largest that is kept
        genes = rng.integers(0, G, T)
        if heavy[c]:
            genes[0] = G - 1
        x[:, c] = np.bincount(genes, minlength=G)
    if big and C > 4:
        x[G // 2, 4] += 70000
    tot = x.sum(0)
    assert ((tot > TARGET) == heavy).all() and x.max() < 256 + 70000 * big
    return x


def reference(x, target, seed):
    """(the host function's result, numpy's key and pos before, key and pos after) from np.random.seed(seed)."""
    saved = np.random.get_state()
    try:
        np.random.seed(seed)
        s0 = np.random.get_state()
        want = gcommon.downsample(pd.DataFrame(x), target).to_numpy()
        s1 = np.random.get_state()
    finally:
        np.random.set_state(saved)
    return want, (np.array(s0[1], np.uint32), int(s0[2])), (np.array(s1[1], np.uint32), int(s1[2]))


def host_form_words(x, in_name, out_name, target, state):
    dt, code = IN[in_name]
    xt = np.ascontiguousarray(x.astype(dt))
    G, C = xt.shape
    out = np.empty((G, C), OUT[out_name][0])
    key, pos, words = state[0].copy(), ctypes.c_int32(state[1]), ctypes.c_int64(-1)
    _lib.check(_lib.lib().cyto_downsample(G, C, xt.ctypes.data, C, code, out.ctypes.data, C, OUT[out_name][1], target,
                                          key.ctypes.data_as(U32P), ctypes.byref(pos), ctypes.byref(words), 0))
    return words.value, out


class Call:
    """One cyto_downsample_dev call: x uploaded in x_layout (padding: the type's maximum), out a buffer in out_layout filled with
    FILL bytes.  ldx / ldo / same: overrides for the refusals."""

    def __init__(self, x, in_name, x_layout, out_name, out_layout, target, state, ldx=None, ldo=None, same=False):
        dt, code = IN[in_name]
        odt, ocode = OUT[out_name]
        G, C = x.shape
        self.G, self.C, self.odt = G, C, odt
        self.xh, xlead, xld = LY.build(x.astype(dt), x_layout, 4, np.nan)
        assert np.array_equal(LY.extract(self.xh, xlead, xld, G, C), x)           # (the values fit the type)
        self.old, self.olead = LY.pitch_and_lead(C, out_layout, 4)
        self.oh = np.full((self.olead + G * self.old + LY.TAIL) * np.dtype(odt).itemsize, FILL, np.uint8)
        self.key, pos, words = state[0].copy(), ctypes.c_int32(state[1]), ctypes.c_int64(-1)
        xb, ob = _lib.DeviceBuffer.from_numpy(self.xh), _lib.DeviceBuffer.from_numpy(self.oh)
        try:
            xp = xb.ptr + xlead * self.xh.itemsize
            op = xp if same else ob.ptr + self.olead * np.dtype(odt).itemsize
            self.status = _lib.lib().cyto_downsample_dev(G, C, xp, xld if ldx is None else ldx, code, op, self.old if ldo is None else ldo,
                                                         ocode, target, self.key.ctypes.data_as(U32P), ctypes.byref(pos),
                                                         ctypes.byref(words), 0)
            self.out_bytes = ob.to_numpy(self.oh.shape, np.uint8)
            self.x_after = xb.to_numpy(self.xh.shape, self.xh.dtype)
        finally:
            xb.free()
            ob.free()
        self.pos, self.words = pos.value, words.value

    def block(self):
        return LY.extract(self.out_bytes.view(self.odt), self.olead, self.old, self.G, self.C)

    def outside_untouched(self):
        mask = np.repeat(LY.data_mask(self.G, self.C, self.olead, self.old), np.dtype(self.odt).itemsize)
        return bool((self.out_bytes[~mask] == FILL).all())

    def input_untouched(self):
        return np.array_equal(self.x_after.view(np.uint8), self.xh.view(np.uint8))

    def nothing_written(self):
        return bool((self.out_bytes == FILL).all())


_REF = {}


def _case(G, C, seed, big=False):
    key = (G, C, seed, big)
    if key not in _REF:
        x = counts(G, C, seed, big=big)
        _REF[key] = (x,) + reference(x, TARGET, seed)
    return _REF[key]


def check(tag, x, want, s0, s1, in_name, x_layout, out_name, out_layout, target=TARGET, words=None):
    """The four assertions of the module's docstring; returns the failures."""
    c = Call(x, in_name, x_layout, out_name, out_layout, target, s0)
    fails = []
    if c.status != 0:
        return [f"{tag}: status {c.status}"]
    got = c.block()
    if not np.array_equal(LY.bits(got), LY.bits(want.astype(c.odt))):
        bad = np.flatnonzero((got != want).any(0))
        fails.append(f"{tag}: {len(bad)} cells differ from numpy's (first: {bad[:6]})")
    if not np.array_equal(c.key, s1[0]) or c.pos != s1[1]:
        fails.append(f"{tag}: the generator's state differs from numpy's (pos {c.pos}, numpy {s1[1]})")
    if words is not None and c.words != words:
        fails.append(f"{tag}: words_out {c.words}, the host form {words}")
    if not c.outside_untouched():
        fails.append(f"{tag}: bytes of the output buffer outside the block were written")
    if not c.input_untouched():
        fails.append(f"{tag}: the input buffer changed")
    return fails


def _report(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:20])


def _assert_mixture(x, G, C):
    heavy = x.sum(0) > TARGET
    if C > 1:
        assert 3 * heavy.sum() >= C and 3 * (~heavy).sum() >= C and heavy[0] != heavy[C - 1]
    if G == 2049 and heavy.any():                         # (all but the one light cell of C = 1)
        assert (x[2048:, heavy].sum(0) > 0).any()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_every_layout_of_x_and_of_out(pair):
    x_layout, out_layout = pair
    assert {p[0] for p in PAIRS} == set(LY.LAYOUTS) and {p[1] for p in PAIRS} == set(OUT_LAYOUTS)
    G, C = 513, 257
    x, want, s0, s1 = _case(G, C, 11)
    _assert_mixture(x, G, C)
    fails = []
    for in_name, out_name in (("int64", "int64"), ("uint8", "uint16"), ("uint16", "int64")):
        words, host_out = host_form_words(x, in_name, out_name, TARGET, s0)
        assert words > 0 and np.array_equal(host_out, want)
        fails += check(f"{in_name}->{out_name} x {x_layout} out {out_layout}", x, want, s0, s1, in_name, x_layout, out_name, out_layout,
                       words=words)
    _report(fails)


@pytest.mark.parametrize("out_name", list(OUT))
@pytest.mark.parametrize("in_name", list(IN))
def test_every_input_and_output_type(in_name, out_name):
    G, C = 513, 257
    big = in_name in ("int32", "int64")
    x, want, s0, s1 = _case(G, C, 12, big)
    _assert_mixture(x, G, C)
    assert not big or x.max() > 65535
    words, _ = host_form_words(x, in_name, out_name, TARGET, s0)
    _report(check(f"{in_name}->{out_name}", x, want, s0, s1, in_name, "odd_pitch", out_name, "offset_base", words=words) +
            check(f"{in_name}->{out_name}", x, want, s0, s1, in_name, "quad_offset_base", out_name, "wide", words=words))


@pytest.mark.parametrize("C", [1, 255, 257])
@pytest.mark.parametrize("G", [1, 511, 513, 2049])
def test_shapes_at_which_the_kernels_loops_change(G, C):
    """TOT_SLAB = 512 genes a workgroup in ds_totals, HIST_CH = 2048 genes a chunk in ds_hist, 256 columns a workgroup.  One cell
    (C = 1) cannot be one of each kind: it is run once heavy and once light."""
    fails = []
    instances = [_case(G, C, 100 + G + C)]
    if C == 1:
        light = counts(G, 1, 7, heavy=np.array([False]))
        instances.append((light,) + reference(light, TARGET, 7))
        assert instances[0][0].sum() > TARGET >= light.sum()
    for x, want, s0, s1 in instances:
        _assert_mixture(x, G, C)
        for in_name, x_layout, out_name, out_layout in (("uint16", "odd_pitch", "int64", "wide"), ("uint8", "offset_base", "uint16", "odd_pitch"),
                                                        ("int64", "wide", "int64", "offset_base")):
            words, _ = host_form_words(x, in_name, out_name, TARGET, s0)
            fails += check(f"G={G} C={C} {in_name} {x_layout} -> {out_name} {out_layout}", x, want, s0, s1, in_name, x_layout, out_name,
                           out_layout, words=words)
    _report(fails)


def test_all_cells_under_the_target_are_copied_and_no_word_is_drawn():
    G, C = 513, 257
    x = counts(G, C, 13, heavy=np.zeros(C, bool))
    want, s0, s1 = reference(x, TARGET, 13)
    assert np.array_equal(want, x) and np.array_equal(s0[0], s1[0]) and s0[1] == s1[1]
    fails = []
    for x_layout, out_layout in PAIRS:
        fails += check(f"x {x_layout} out {out_layout}", x, want, s0, s1, "uint16", x_layout, "int64", out_layout, words=0)
    # a negative count in a cell that is kept is copied (int64 output)
    x[5, 3] -= 400
    x[6, 3] += 350
    assert x[5, 3] < 0 and x[:, 3].sum() <= TARGET
    want, s0, s1 = reference(x, TARGET, 13)
    fails += check("a kept negative count", x, want, s0, s1, "int32", "odd_pitch", "int64", "wide", words=0)
    _report(fails)


def test_target_zero():
    G, C = 513, 257
    x = counts(G, C, 14)
    want, s0, s1 = reference(x, 0, 14)
    assert not want.any() and x.any() and np.array_equal(s0[0], s1[0]) and s0[1] == s1[1]
    fails = []
    for in_name, x_layout, out_name, out_layout in (("uint8", "odd_pitch", "uint16", "offset_base"), ("int64", "offset_base", "int64", "odd_pitch")):
        fails += check(f"target 0 {in_name}->{out_name}", x, want, s0, s1, in_name, x_layout, out_name, out_layout, target=0, words=0)
    _report(fails)


def test_refusals_leave_the_output_and_the_state_alone():
    G, C = 513, 257
    x, _, s0, _ = _case(G, C, 11)
    neg = x.copy()
    neg[7, 0] = -1
    neg[8, 0] += 1
    assert neg[:, 0].sum() > TARGET
    ld, _ = LY.pitch_and_lead(C, "odd_pitch", 4)
    assert ld > C
    cases = {
        "x_dev == out_dev": dict(x=x, in_name="int64", out_name="int64", same=True),
        "ldx < C": dict(x=x, in_name="uint16", out_name="int64", ldx=C - 1),
        "ldo < C": dict(x=x, in_name="uint16", out_name="int64", ldo=C - 1),
        "a negative count in a downsampled cell": dict(x=neg, in_name="int32", out_name="int64"),
        "a negative count in a downsampled cell (int64)": dict(x=neg, in_name="int64", out_name="uint16"),
        "uint16 output with target > 65535": dict(x=x, in_name="uint16", out_name="uint16", target=65536),
    }
    for name, kw in cases.items():
        kw = dict(kw)
        c = Call(kw.pop("x"), kw.pop("in_name"), "odd_pitch", kw.pop("out_name"), "odd_pitch", kw.pop("target", TARGET), s0, **kw)
        assert c.status == 1, (name, c.status)
        assert c.nothing_written(), name
        assert c.input_untouched(), name
        assert np.array_equal(c.key, s0[0]) and c.pos == s0[1], name
    # the control: the same call with nothing wrong is accepted
    assert Call(x, "uint16", "odd_pitch", "int64", "odd_pitch", TARGET, s0).status == 0


def test_poisoned_work_buffers_change_nothing():
    G, C = 2049, 257
    x, want, s0, s1 = _case(G, C, 100 + G + C)
    words, _ = host_form_words(x, "uint16", "int64", TARGET, s0)
    _lib.cache_poison(FILL)
    try:
        f0 = _lib.cache_poison_fills()
        fails = check("poisoned", x, want, s0, s1, "uint16", "odd_pitch", "int64", "offset_base", words=words)
        assert _lib.cache_poison_fills() > f0
        fails += check("poisoned uint16", x, want, s0, s1, "uint8", "offset_base", "uint16", "wide", words=words)
    finally:
        _lib.cache_poison(None)
    _report(fails)
