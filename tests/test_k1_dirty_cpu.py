"""stage_u1t_kernel's neighbourhood test on one-hot MSB masks and its one-operation sort keys, on the CPU (no GPU): mulut_core.h's
tube1_span_gt1 / tube1_dirty4 / tube1_key compiled with g++ from tests/host_emul/emul_k1_dirty.cpp.  Bar: the verdict of every union
mask and of every window equals the max - min definition; the key expression equals the three-input truth table the device uses.
Also asserted here, on the oracle alone: what the crafted frames of tests/test_gpu_k1_diet.py hold, and that a missed flag would
change their bytes."""
import ctypes

import numpy as np
import pytest

import k1_diet_cases as K
from host_emul_lib import load_emul
from oracle import c_oracle


@pytest.fixture(scope="module")
def lib():
    lib = load_emul("emul_k1_dirty", ["mulut_core.h"])
    lib.k1_span_gt1.argtypes = [ctypes.c_uint32]
    lib.k1_span_gt1.restype = ctypes.c_uint32
    lib.k1_onehot.argtypes = [ctypes.c_uint32]
    lib.k1_onehot.restype = ctypes.c_uint32
    lib.k1_dirty_windows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.k1_dirty_windows.restype = None
    lib.k1_key_check.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_long)]
    lib.k1_key_check.restype = ctypes.c_long
    return lib


def test_every_union_mask(lib):
    """All 65,535 non-zero masks, each in the low half beside 65,536 - T in the high half (a carry or a borrow between the halves would show)."""
    bad = 0
    for t in range(1, 65536):
        u = 65536 - t
        got = lib.k1_span_gt1(t | (u << 16))
        want = [int(m.bit_length() - 1 - ((m & -m).bit_length() - 1) > 1) for m in (t, u)]
        bad += got != (want[0] | (want[1] << 16))
    print("union masks wrong:", bad)
    assert bad == 0


def test_onehot_ignores_the_lsb_nibble(lib):
    for h in range(16):
        for f in range(16):
            assert lib.k1_onehot((f << 12 | h) | ((15 - f) << 12 | (15 - h)) << 16) == (1 << h) | (1 << (15 - h)) << 16, (h, f)


@pytest.mark.parametrize("name,h,f", K.windows(), ids=lambda v: v if isinstance(v, str) else "")
def test_windows_against_max_minus_min(lib, name, h, f):
    codes = np.ascontiguousarray((f << 12) | h, np.uint16)
    got = np.zeros(len(codes), np.uint8)
    lib.k1_dirty_windows(codes.ctypes.data, len(codes), got.ctypes.data)
    want = np.array([K.window_dirty(w) for w in h], np.uint8)
    print(name, len(codes), "windows; flagged pixels", int(sum(bin(v).count("1") for v in want)), "of", 4 * len(codes), "; wrong", int((got != want).sum()))
    assert np.array_equal(got, want)
    if name not in ("narrow", "uniform"):       # (one step at most: never flagged; any level anywhere: nearly always)
        assert 0 < sum(bin(v).count("1") for v in want) < 4 * len(codes)        # both verdicts occur
    if name == "single_outlier":        # 40 positions x (one level off: never, two levels off: the pixels within reach)
        assert len(codes) == 40 * (2 + 3 + 4 + 4 + 3 + 2)


@pytest.mark.parametrize("slot", [4, 8, 24])
def test_key_expression_is_truth_table_0xea(lib, slot):
    n = ctypes.c_long(0)
    bad = lib.k1_key_check(slot, ctypes.byref(n))
    print("slot", slot, "keys", n.value, "wrong", bad)
    assert bad == 0 and n.value == 4 * 65536


# ---- the frames of the GPU test, on the oracle alone ------------------------------------------------------------------------------
def tiles(mask_hwc):
    H, W, _ = mask_hwc.shape
    for y0 in range(0, H, K.TILE):
        for x0 in range(0, W, K.TILE):
            yield (y0, x0), mask_hwc[y0:y0 + K.TILE, x0:x0 + K.TILE]


@pytest.mark.parametrize("kind", ["shipped", "seeded"])
@pytest.mark.parametrize("shape", [(K.H_HWC, K.W_HWC), (K.H_PL, K.W_PL)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_frames_hold_dirty_and_clean_sites_and_a_missed_flag_shows(shipped_luts, name, shape, kind):
    """Every tile of every frame holds dirty sites and clean sites.  With the band-aliased tables (no site ever flagged; the slots no
    tube row owns filled with -128 and with 127 in turn) the first stage's bytes equal the oracle's at every clean site and differ at
    dirty ones.  (Low nibbles of 15 give weight to a pass's first and last row only: only the sites around the pixels three levels off
    can differ there.)"""
    x = K.frames(name, *shape)
    luts = shipped_luts if kind == "shipped" else K.seeded_luts()
    t1 = [luts["s1_%s" % m] for m in "sdy"]
    alias = {fill: [K.band_aliased(t, fill) for t in t1] for fill in (-128, 127)}
    differ = 0
    for f in x:
        d = K.dirty_mask(f)
        for where, m in tiles(d):
            assert m.any() and not m.all(), (name, where)
        want = c_oracle.stage(t1, "sdy", False, f, 1)
        shows = np.ones(d.shape, bool)
        for fill in alias:
            got = c_oracle.stage(alias[fill], "sdy", False, f, 1)
            assert np.array_equal(got[~d], want[~d]), name           # clean sites never leave the tube
            shows &= got != want
        differ += int(shows.sum())
        print(name, shape, kind, "dirty sites", int(d.sum()), "of", d.size, "; a missed flag changes the byte at", int(shows.sum()))
    assert differ > 100


def test_levels_dirty_is_the_window_definition():
    rng = np.random.default_rng(3)
    h = rng.integers(5, 9, (12, 19))
    d = K.levels_dirty(h)
    p = np.pad(h, 2, mode="edge")
    for y in range(12):
        for x in range(19):
            w = p[y:y + 5, x:x + 5]
            assert d[y, x] == (w.max() - w.min() > 1)
