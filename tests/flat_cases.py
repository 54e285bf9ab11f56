"""Shared cases and NumPy reference of tests/test_flat_cpu.py and tests/test_gpu_tube2_flat.py (TEST ONLY; NumPy alone).

stage_tube2_kernel skips a channel's per-pass tube tests on a wave tile (16 x 4 sites) whose image of that channel lies on two adjacent
MSB levels.  The reference here gives, for a final-stage input image, the exact per-(pixel, channel) dirty mask (a sample is dirty when
one of its twelve passes has four key MSBs that span more than one step: tools/tube_histogram.py's formula, edge-replicated) and the flat
predicate per (wave tile, channel) over the pixels the tile's windows read.  The kernel may use any superset of those pixels, so what
the reference calls flat the kernel may still test; what the reference calls dirty the kernel must flag, flat or not."""
import numpy as np

PAT = {"s": ((0, 1), (1, 0), (1, 1)), "d": ((0, 2), (2, 0), (2, 2)), "y": ((1, 1), (1, 2), (2, 1))}
TW, TH, HALO = 16, 4, 2         # a wave's tile and the reach of a 5 x 5 window


def _rot(r, di, dj):
    return [(di, dj), (dj, -di), (-di, -dj), (-dj, di)][r]


def _shifted(h, dy, dx):
    H, W = h.shape[:2]
    ys = np.clip(np.arange(H) + dy, 0, H - 1)
    xs = np.clip(np.arange(W) + dx, 0, W - 1)
    return h[ys][:, xs]


def dirty_mask(img_hwc):
    """bool [H][W][C]: the sample has a pass (mode s, d, y x rotation) whose four key MSBs span more than one step."""
    h = (np.asarray(img_hwc, np.uint8) >> 4).astype(np.int16)
    out = np.zeros(h.shape, bool)
    for m in "sdy":
        for r in range(4):
            hs = [h] + [_shifted(h, *_rot(r, di, dj)) for di, dj in PAT[m]]
            out |= (np.maximum.reduce(hs) - np.minimum.reduce(hs)) > 1
    return out


def flat_tiles(img_hwc):
    """bool [tiles_y][tiles_x][C]: the MSBs of the pixels the tile's windows read (rows y0 - 2 .. y0 + 5, columns x0 - 2 .. x0 + 17,
    clamped to the frame) span at most one step."""
    h = (np.asarray(img_hwc, np.uint8) >> 4).astype(np.int16)
    H, W, C = h.shape
    ty, tx = -(-H // TH), -(-W // TW)
    out = np.zeros((ty, tx, C), bool)
    for j in range(ty):
        ys = np.clip(np.arange(j * TH - HALO, j * TH + TH + HALO), 0, H - 1)
        for i in range(tx):
            xs = np.clip(np.arange(i * TW - HALO, i * TW + TW + HALO), 0, W - 1)
            blk = h[ys][:, xs]
            out[j, i] = (blk.max((0, 1)) - blk.min((0, 1))) <= 1
    return out


def dirty_tiles(img_hwc):
    """bool [tiles_y][tiles_x][C]: the tile holds a dirty sample of the channel."""
    d = dirty_mask(img_hwc)
    H, W, C = d.shape
    ty, tx = -(-H // TH), -(-W // TW)
    p = np.zeros((ty * TH, tx * TW, C), bool)
    p[:H, :W] = d
    return p.reshape(ty, TH, tx, TW, C).any((1, 3))


# ---------------------------------------------------------------------------------------------
# the small cases: 40 x 48, constant MSB level with one pixel two steps away, seen from the wave tile at (x0, y0) = (16, 4)
# ---------------------------------------------------------------------------------------------
H0, W0, LEVEL = 40, 48, 7
TILE = (1, 1)                   # (tile row, tile column) of the tile at y0 = 4, x0 = 16
Y0, X0 = 4, 16


def _base(c, seed):
    """MSB level LEVEL everywhere, seeded low nibbles (the interpolation weights: no pass reads a single table row)."""
    rng = np.random.default_rng([seed, c])
    return (LEVEL * 16 + rng.integers(0, 16, (H0, W0, c))).astype(np.uint8)


def outlier(y, x, c=3, channels=None, seed=0):
    img = _base(c, seed)
    for ch in (range(c) if channels is None else channels):
        img[y, x, ch] = (LEVEL + 2) * 16 + (img[y, x, ch] & 15)
    return img


def checker(c=3, seed=1, site=None):
    """MSBs LEVEL and LEVEL + 1 in a checker: every tile flat, no dirty sample; `site` = (y, x) puts one pixel at LEVEL + 2."""
    img = _base(c, seed)
    yy, xx = np.mgrid[0:H0, 0:W0]
    img += (((yy + xx) & 1) * 16).astype(np.uint8)[..., None]
    if site is not None:
        img[site[0], site[1]] = (LEVEL + 2) * 16 + (img[site[0], site[1]] & 15)
    return img


# name -> (image, channels that hold the outlier, expectation for the tile at (16, 4): "dirty", "flat" or None = not about that tile)
def small_cases():
    cases = {"inside": (outlier(Y0 + 1, X0 + 4), (0, 1, 2), "dirty")}
    for dx in (-2, -1, 16, 17):
        cases["halo_col%+d" % dx] = (outlier(Y0 + 1, X0 + dx), (0, 1, 2), "dirty")
    for dy in (-2, -1, 4, 5):
        cases["halo_row%+d" % dy] = (outlier(Y0 + dy, X0 + 4), (0, 1, 2), "dirty")
    for name, (dy, dx) in {"outside_col-3": (1, -3), "outside_col+18": (1, 18), "outside_row-3": (-3, 4), "outside_row+6": (6, 4)}.items():
        cases[name] = (outlier(Y0 + dy, X0 + dx), (0, 1, 2), "flat")
    cases["channel1_only"] = (outlier(Y0 + 1, X0 + 4, channels=(1,)), (1,), "dirty")
    cases["channel2_only"] = (outlier(Y0 + 1, X0 + 4, channels=(2,)), (2,), "dirty")       # (its first two pairs are indexed inside channel 1)
    cases["C1"] = (outlier(Y0 + 1, X0 + 4, c=1), (0,), "dirty")
    cases["C2"] = (outlier(Y0 + 1, X0 + 4, c=2), (0, 1), "dirty")
    cases["C2_channel1_only"] = (outlier(Y0 + 1, X0 + 4, c=2, channels=(1,)), (1,), "dirty")
    cases["two_level"] = (checker(), (), "flat")
    cases["two_level_one_site"] = (checker(site=(Y0 + 2, X0 + 9)), (0, 1, 2), "dirty")
    for name, (y, x) in {"border_row0": (0, 21), "border_col0": (13, 0), "border_last_row": (H0 - 1, 30), "border_last_col": (22, W0 - 1),
                         "border_corner": (H0 - 1, W0 - 1)}.items():
        cases[name] = (outlier(y, x), (0, 1, 2), None)
    return cases


OUTLIER_AT = {"inside": (Y0 + 1, X0 + 4), "channel1_only": (Y0 + 1, X0 + 4), "channel2_only": (Y0 + 1, X0 + 4), "C1": (Y0 + 1, X0 + 4),
              "C2": (Y0 + 1, X0 + 4), "C2_channel1_only": (Y0 + 1, X0 + 4), "two_level_one_site": (Y0 + 2, X0 + 9),
              "border_row0": (0, 21), "border_col0": (13, 0), "border_last_row": (H0 - 1, 30), "border_last_col": (22, W0 - 1),
              "border_corner": (H0 - 1, W0 - 1), "outside_col-3": (Y0 + 1, X0 - 3), "outside_col+18": (Y0 + 1, X0 + 18),
              "outside_row-3": (Y0 - 3, X0 + 4), "outside_row+6": (Y0 + 6, X0 + 4)}
OUTLIER_AT.update({"halo_col%+d" % dx: (Y0 + 1, X0 + dx) for dx in (-2, -1, 16, 17)})
OUTLIER_AT.update({"halo_row%+d" % dy: (Y0 + dy, X0 + 4) for dy in (-2, -1, 4, 5)})


# ---------------------------------------------------------------------------------------------
# persistent waves on partial tiles: more work items than a launch has waves, a frame width and height that are no multiple of the tile
# ---------------------------------------------------------------------------------------------
def ridged(n, h, w, c, seed=0):
    """A smooth field (one MSB step over ~90 pixels) with steep two-pixel ridges, three MSB steps high, on diagonals that cross every
    tile row and column, plus one along the right and one along the bottom edge: the partial tiles there and the full tiles around them
    all carry dirty samples.  uint8 [n][h][w][c]."""
    rng = np.random.default_rng([seed, n, h, w, c])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((n, h, w, c), np.uint8)
    for f in range(n):
        for ch in range(c):
            ph = rng.uniform(0, 2 * np.pi, 2)
            v = 104 + 28 * np.sin(xx / 57.0 + ph[0]) * np.cos(yy / 43.0 + ph[1]) + rng.uniform(0, 6, (h, w))
            k = 37 + 6 * ch + 11 * f
            ridge = (((xx + 3 * yy + k) % 97) < 2) | (((3 * xx - yy + k) % 211) < 2) | (np.abs(xx - (w - 3)) < 1) | (np.abs(yy - (h - 2)) < 1)
            out[f, :, :, ch] = np.clip(v + 48 * ridge, 0, 255).astype(np.uint8)
    return out


PARTIAL_SHAPES = [(2, 144, 1000, 3), (2, 142, 1000, 3)]      # 288 verdict tiles (64 x 16), W % 16 = 8; rows % 4 = 2
