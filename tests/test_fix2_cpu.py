"""stage_up_fix2_kernel's body for lists of up to four modes on the CPU (no GPU): mulut_core.h's packed row sums (fix2_mac_row,
fix2_pass_sums), the placement of a pass in a group's two accumulator sets (fix2_slot, fix2_swap), the finishing map (fix2_partner,
fix2_field_half) and the entry decode by reciprocals (Recip30, fix2_decode), compiled with g++ from tests/host_emul/emul_fix2.cpp
and run lane by lane as the kernel runs them.  Bar: the sixteen bytes of a sample's block equal the C oracle's; every decoded id
equals divmod."""
import ctypes

import numpy as np
import pytest

import fix2_cases as X
from host_emul_lib import load_emul
from oracle import c_oracle


@pytest.fixture(scope="module")
def lib():
    L = load_emul("emul_fix2", ["mulut_core.h"])
    L.fix2_sample.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 5
    L.fix2_sample.restype = None
    L.fix2_decode_check.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    L.fix2_decode_check.restype = ctypes.c_long
    L.fix2_recip.argtypes = [ctypes.c_uint32, ctypes.c_void_p]
    L.fix2_recip.restype = None
    return L


H, W = 9, 11
SITES = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (1, 1), (4, 5), (2, W - 2), (H - 2, 3), (3, 0), (0, 6)]      # corners, edges (the clamps), inside


def run_samples(lib, modes, tables, img):
    """Blocks [site][4][4] of the emulated lanes, with the peak LDS field and the range of the finishing sums over the sites."""
    dev = [np.ascontiguousarray((t.astype(np.int16) + 128).astype(np.uint8)) for t in tables]      # the device format: value + 128
    ptrs = (ctypes.c_void_p * len(dev))(*[t.ctypes.data for t in dev])
    di = np.ascontiguousarray([[d[0] for d in X.PAT[m]] for m in modes], np.int32)
    dj = np.ascontiguousarray([[d[1] for d in X.PAT[m]] for m in modes], np.int32)
    img = np.ascontiguousarray(img, np.uint8)
    blocks, peak, lo, hi = [], 0, 1 << 30, 0
    for y, x in SITES:
        out, info = np.zeros(16, np.uint8), np.zeros(3, np.int32)
        lib.fix2_sample(img.ctypes.data, H, W, y, x, len(modes), ptrs, di.ctypes.data, dj.ctypes.data, out.ctypes.data, info.ctypes.data)
        blocks.append(out.reshape(4, 4))
        peak, lo, hi = max(peak, int(info[0])), min(lo, int(info[1])), max(hi, int(info[2]))
    return np.stack(blocks), peak, lo, hi


def oracle_blocks(modes, tables, img):
    want = c_oracle.stage(tables, modes, True, img[..., None], 4)[..., 0]
    return np.stack([want[4 * y:4 * y + 4, 4 * x:4 * x + 4] for y, x in SITES])


@pytest.mark.parametrize("modes", ["sdy", "ysd", "s", "sd", "sdys"])
@pytest.mark.parametrize("seed", range(4))
def test_random_tables_give_the_oracles_block(lib, modes, seed):
    tables = [X.final_table("random", m, seed) for m in modes]
    img = X.noise(1, H, W, 1, seed)[0, :, :, 0]
    got, peak, lo, hi = run_samples(lib, modes, tables, img)
    want = oracle_blocks(modes, tables, img)
    print(modes, seed, "peak field", peak, "sums", lo, hi, "differing bytes", int((got != want).sum()))
    assert np.array_equal(got, want)
    assert len(np.unique(want)) > 8          # the blocks are not clipped flat: a misplaced element changes a byte


@pytest.mark.parametrize("kind", ["max", "min", "alt", "alt_c"])
def test_extreme_tables_at_four_modes(lib, kind):
    """All +127: every finishing sum is 4 M x 4080 = 65,280, a set's field 32,640 -- the bound, hit exactly.  All -128: every
    field 0.  +127 / -128 alternating per element: inside a pass the odd bytes are 255 beside even bytes of 0 (alt_c) or the other
    way round, so the raw-dword sums F wrap mod 2^16 (256 x 4080) and the even fields must come back as exactly 0, or 4080 beside
    H = 0.  A quarter turn moves even elements to odd positions and a half turn keeps them, so every field of a set ends at
    M x 4080 = 16,320 and every finishing sum at 32,640 (K = -128, byte 0): a carry or a lost wrap changes those numbers."""
    modes = "sdys"
    tables = [X.final_table(kind, m) for m in modes]
    img = X.noise(1, H, W, 1, 7)[0, :, :, 0]
    got, peak, lo, hi = run_samples(lib, modes, tables, img)
    want = oracle_blocks(modes, tables, img)
    print(kind, "peak field", peak, "sums", lo, hi, "differing bytes", int((got != want).sum()))
    assert np.array_equal(got, want)
    if kind == "max":
        assert (peak, lo, hi) == (32640, 65280, 65280) and (got == 255).all()
    if kind == "min":
        assert (peak, lo, hi) == (0, 0, 0) and (got == 0).all()
    if kind.startswith("alt"):
        assert (peak, lo, hi) == (16320, 32640, 32640) and (got == 0).all()


def test_every_rotation_puts_every_element_where_the_oracle_does(lib):
    """Tables of zeros with row element e alone at +127, on a flat image (weight 16 on one row): the pass of rotation r adds
    255 x 16 at the one block position it gives element e and 128 x 16 elsewhere, so the block is 127 at the four positions the
    four rotations give e and 0 at the other twelve.  A slot, a half swap or a partner field that is off moves one of them."""
    img = np.full((H, W), 64, np.uint8)
    for e in range(16):
        t = np.zeros((17 ** 4, 16), np.int8)
        t[:, e] = 127
        got, _, _, _ = run_samples(lib, "s", [t], img)
        want = oracle_blocks("s", [t], img)
        assert np.array_equal(got, want), e
        assert sorted(np.unique(want[4])) == [0, 127] and (want[4] == 127).sum() == 4, e


DECODE = [(1, 5), (3, 21), (37, 21), (1000, 1000), (1920, 1080), (7680, 4320), (65535, 16384), (65535, 1)]


@pytest.mark.parametrize("wh", DECODE, ids=lambda p: "%dx%d" % p)
def test_decode_equals_divmod(lib, wh):
    w, h = wh
    info = np.zeros(3, np.uint32)
    bad = lib.fix2_decode_check(w, h, info.ctypes.data)
    checked = int(info[1]) | (int(info[2]) << 32)
    print("W", w, "H", h, "multiply-high form" if info[0] else "plain division", "ids checked", checked, "wrong", bad)
    assert bad == 0
    assert checked >= (1 if w == 1 else 2) * ((1 << 30) // w)
    assert bool(info[0]) == (w >= 2)            # a divisor of 1 has no 32-bit magic: those launches keep the division


def test_reciprocal_is_exact_for_every_divisor_shape(lib):
    """magic = ceil(2^(32 + s) / d) with s = floor(log2 d) - 1, in Python integers: it fits 32 bits and its error stays below the
    bound for ids < 2^30, for powers of two, their neighbours and the largest divisors."""
    ds = sorted({d for k in range(1, 31) for d in (2 ** k - 1, 2 ** k, 2 ** k + 1)} | {3, 37, 1000, 1920, 7680, 65535, 2 ** 30 - 1, 2 ** 31 + 5, 2 ** 32 - 1})
    for d in ds:
        if d < 2:
            continue
        out = np.zeros(3, np.uint32)
        lib.fix2_recip(d, out.ctypes.data)
        s = d.bit_length() - 2
        m = -((-(1 << (32 + s))) // d)
        assert (int(out[0]), int(out[1]), int(out[2])) == (m, s, 1), d
        assert m < 2 ** 32 and (m * d - (1 << (32 + s))) * (2 ** 30 - 1) < (1 << (32 + s))
    for d in (0, 1):
        out = np.ones(3, np.uint32)
        lib.fix2_recip(d, out.ctypes.data)
        assert int(out[2]) == 0
