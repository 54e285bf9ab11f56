"""Shared cases and NumPy reference of tests/test_k1_dirty_cpu.py and tests/test_gpu_k1_diet.py (TEST ONLY; NumPy alone).

stage_u1t_kernel flags a site when the 5 x 5 neighbourhood of its pixel (edge-replicated) spans more than one MSB step; a flagged site
is recomputed from the full table, an unflagged one keeps what the tube band gave.  The reference here is that predicate by max - min,
the crafted inputs of the GPU test, and the band-aliased tables that tell on the CPU whether a missed flag could show in a case's bytes."""
import numpy as np

L, HALO = 17, 2
TILE = 64                       # stage_u1t_kernel's tile edge
SA, SB, SC, SD = 27, 18, 12, 8  # tube slot strides (mulut_core.h: kTubeSA ..), 1041 slots
SLOTS = 16 * (SA + SB + SC + SD) + 1
H_HWC, W_HWC = 70, 134          # two tile rows, three tile columns, the last one 6 pixels wide; W % 4 != 0: the kernel's byte path
H_PL, W_PL = 66, 128            # planar input with W % 4 == 0: its dword path


def levels_dirty(h):
    """bool like h: the 5 x 5 neighbourhood (edge-replicated) of the MSB levels h [..., H, W] spans more than one step, by max - min."""
    h = np.asarray(h, np.int16)
    H, W = h.shape[-2:]
    hi, lo = h.copy(), h.copy()
    for dy in range(-HALO, HALO + 1):
        ys = np.clip(np.arange(H) + dy, 0, H - 1)
        for dx in range(-HALO, HALO + 1):
            xs = np.clip(np.arange(W) + dx, 0, W - 1)
            s = h[..., ys, :][..., xs]
            hi, lo = np.maximum(hi, s), np.minimum(lo, s)
    return (hi - lo) > 1


def dirty_mask(img_hwc):
    """bool [H][W][C] of a uint8 frame."""
    return levels_dirty((np.asarray(img_hwc, np.uint8) >> 4).transpose(2, 0, 1)).transpose(1, 2, 0)


# ---------------------------------------------------------------------------------------------
# windows of the CPU test: codes f << 12 | h, 5 rows x 8 columns (a thread's four pixels sit at columns 2 .. 5)
# ---------------------------------------------------------------------------------------------
def window_dirty(h58):
    """four bits of a [5][8] level window by max - min: bit i = columns i .. i + 4 span more than one step"""
    h = np.asarray(h58, np.int16)
    return sum(((int(h[:, i:i + 5].max()) - int(h[:, i:i + 5].min())) > 1) << i for i in range(4))


def windows():
    """(name, h [n][5][8], f [n][5][8]): seeded windows that wander by at most one step around a level (few flags) or over three levels
    (most flags), every single-outlier placement one and two levels off, windows at the rims h = 0 and h = 15, and f = 15 everywhere."""
    rng = np.random.default_rng(20)
    out = []
    n = 3000
    base = rng.integers(0, 16, (n, 1, 1))
    narrow = np.clip(base + rng.integers(0, 2, (n, 5, 8)), 0, 15)
    wide = np.clip(base + rng.integers(-1, 2, (n, 5, 8)) * (rng.random((n, 5, 8)) < 0.15), 0, 15)
    anyh = rng.integers(0, 16, (n // 10, 5, 8))
    for name, h in (("narrow", narrow), ("wide", wide), ("uniform", anyh)):
        out.append((name, h, rng.integers(0, 16, h.shape)))
    single = []
    for level in (0, 1, 7, 13, 14, 15):
        for off in (-2, -1, 1, 2):
            if not 0 <= level + off <= 15:
                continue
            for p in range(40):
                w = np.full((5, 8), level)
                w[p // 8, p % 8] = level + off
                single.append(w)
    single = np.stack(single)
    out.append(("single_outlier", single, rng.integers(0, 16, single.shape)))
    rims = np.concatenate([rng.integers(0, 2, (300, 5, 8)) * 15, rng.integers(0, 3, (300, 5, 8)), 15 - rng.integers(0, 3, (300, 5, 8)),
                           np.zeros((1, 5, 8), np.int64), np.full((1, 5, 8), 15)])
    out.append(("rims", rims, rng.integers(0, 16, rims.shape)))
    f15 = np.concatenate([narrow[:500], wide[:500], single, rims])
    out.append(("f15", f15, np.full(f15.shape, 15)))
    return out


# ---------------------------------------------------------------------------------------------
# frames of the GPU test
# ---------------------------------------------------------------------------------------------
def _lsb(h, w, c):
    """a smooth ramp of the low nibbles, another per channel (the interpolation weights: no pass reads a single table row)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([((xx + 2 * yy + 5 * ch) // 3) % 16 for ch in range(c)], -1)


def _frame(levels, lsb):
    return (np.asarray(levels) * 16 + lsb).astype(np.uint8)


def edges(h, w):
    """(a) one MSB level with straight edges of one step (no site dirty) and of two steps (the sites within two pixels dirty): vertical
    ones every 13 columns in channel 0 (13 k runs through every column phase mod 4), horizontal ones every 9 rows in channel 1,
    diagonal ones of both directions in channel 2; the step is one level or two by a 20-pixel checkerboard of zones, so every tile
    -- the narrow last column too, in the frame and in its mirror image -- holds both kinds."""
    yy, xx = np.mgrid[0:h, 0:w]
    step = 1 + (xx // 20 + yy // 20) % 2
    lv = np.empty((h, w, 3), np.int64)
    lv[..., 0] = 7 + ((xx // 13) % 2) * step
    lv[..., 1] = 7 + ((yy // 9) % 2) * step
    lv[..., 2] = 7 + np.where(xx < w // 2, ((xx + yy) // 11) % 2, ((xx - yy + h) // 11) % 2) * step
    return _frame(lv, _lsb(h, w, 3))


def _grid_sites(h, w):
    """isolated sites 7 apart (coprime to the four-pixel group and to the tile): every column and row phase, the frame's first row and
    column; the last column when w = 7 k + 1; plus the last row and the corners"""
    sites = [(y, x) for y in range(0, h, 7) for x in range(0, w, 7)]
    sites += [(h - 1, x) for x in range(3, w, 7)] + [(h - 1, w - 1), (0, w - 1)]
    return sorted(set(sites))


def isolated(h, w, lsb15=False):
    """(b), (c) level 7 with single pixels two levels off, up and down in turn, 7 apart: each makes the 25 sites around it dirty, every one
    of which sees it at another of the 25 neighbourhood offsets, and leaves clean sites between the blocks.  Every fourth one is three
    levels off: with equal low nibbles a pass weighs its first and last row only, which stay inside the tube (rows of span <= 2) at two
    levels -- only the length of the fix-up list tells on a missed flag there -- and leave it at three.  lsb15: every low nibble 15."""
    lv = np.full((h, w, 3), 7, np.int64)
    for k, (y, x) in enumerate(_grid_sites(h, w)):
        off = 3 if k % 4 == 3 else 2
        lv[y, x, :] = 7 + off if k % 2 == 0 else 7 - off
        lv[y, x, k % 3] = 7 if k % 5 == 4 else lv[y, x, k % 3]      # some sites in two channels only
    return _frame(lv, 15 if lsb15 else _lsb(h, w, 3))


def rims(h, w):
    """(d) the lowest and the highest levels: level 0 with single pixels at 1 (clean) and 2 (dirty) in the upper half, level 15 with single
    pixels at 14 and 13 in the lower half; columns 40 .. 59 alternate 0 / 1 resp. 14 / 15 per pixel (clean)."""
    lv = np.zeros((h, w, 3), np.int64)
    lv[h // 2:] = 15
    yy, xx = np.mgrid[0:h, 0:w]
    chk = ((yy + xx) & 1)[:, 40:60, None]
    lv[:, 40:60] = np.where(lv[:, 40:60] == 0, chk, 15 - chk)
    for k, (y, x) in enumerate(_grid_sites(h, w)):
        if 38 <= x < 62:
            continue
        step = 1 + k % 2
        lv[y, x] = step if y < h // 2 else 15 - step
    return _frame(lv, _lsb(h, w, 3))


CASES = {"edges": edges, "isolated": isolated, "isolated_lsb15": lambda h, w: isolated(h, w, True), "rims": rims}


def frames(name, h, w, n=2):
    """uint8 [n][h][w][3]: the case and, as a second frame, its mirror image (the narrow last tile column then holds the other side)"""
    f = CASES[name](h, w)
    return np.stack([f, f[:, ::-1]][:n])


# ---------------------------------------------------------------------------------------------
# what a missed flag would give
# ---------------------------------------------------------------------------------------------
def band_aliased(table, fill):
    """The table a tube-band kernel would compute with if no site were ever flagged: row (A, B, C, D) replaced by the row at tube slot
    27 A + 18 B + 12 C + 8 D -- itself for the 991 rows inside the tube (max - min of the row's keys <= 2: what a pass whose four MSBs
    span at most one step can touch), some other row outside it, `fill` where no tube row owns the slot.  int8 [17^4][v] -> the same shape."""
    t = np.asarray(table, np.int8).reshape(L, L, L, L, -1)
    a, b, c, d = np.indices((L, L, L, L))
    slot = SA * a + SB * b + SC * c + SD * d
    tube = (np.maximum.reduce([a, b, c, d]) - np.minimum.reduce([a, b, c, d])) <= 2
    assert int(tube.sum()) == 991 and len(np.unique(slot[tube])) == 991          # the slot map is injective on the tube
    band = np.full((SLOTS, t.shape[-1]), fill, np.int8)
    band[slot[tube]] = t[tube]
    out = band[slot]
    assert np.array_equal(out[tube], t[tube])
    return out.reshape(L ** 4, -1)


def seeded_luts(seed=11):
    """a 2-stage x4 cascade of uniformly random int8 tables: whatever row a pass reads in place of its own, the byte changes"""
    rng = np.random.default_rng([seed, 2, 4])
    return {"s%d_%s" % (s, m): rng.integers(-128, 128, (L ** 4, 1 if s == 1 else 16)).astype(np.int8) for s in (1, 2) for m in "sdy"}


def config5_luts(stages=4, scale=2):
    """The seeded synthetic tables of the benchmark's 4-stage x2 cascade (same generator, same draw order), as a lut_dict."""
    rng = np.random.default_rng(5)
    out = {}
    for s in range(1, stages + 1):
        for m in "sdy":
            vn = scale * scale if s == stages else 1
            base = rng.integers(-20, 21, (17, 17, 17, 17, vn)).astype(np.float32)
            grid = np.indices((17, 17, 17, 17)).astype(np.float32).sum(0)[..., None] * (3.0 if s < stages else 4.0) - 96.0
            out["s%d_%s" % (s, m)] = np.clip(np.rint(grid + base), -127, 127).astype(np.int8).reshape(-1, vn)
    return out


def final_luts(scale, seed):
    """one final stage of `scale`: seeded rows around a ramp over the key sum, as config5_luts draws them"""
    rng = np.random.default_rng([seed, scale])
    out = {}
    for m in "sdy":
        base = rng.integers(-20, 21, (17, 17, 17, 17, scale * scale)).astype(np.float32)
        grid = np.indices((17, 17, 17, 17)).astype(np.float32).sum(0)[..., None] * 4.0 - 96.0
        out["s1_%s" % m] = np.clip(np.rint(grid + base), -127, 127).astype(np.int8).reshape(-1, scale * scale)
    return out
