"""Shared cases and NumPy reference of tests/test_fix2_skip_cpu.py and tests/test_gpu_fix2_skip.py (TEST ONLY; NumPy alone).

stage_up_fix2_kernel leaves a listed sample alone when a tube kernel listed it (an entry that names one channel) and all its passes
have their four pixel VALUES within 32 levels: every table row such a pass weighs is a row of the tube band, so the bytes the tube
kernel stored are exact.  Here: the frames that hold both kinds of flagged samples, the masks that say which is which, and the tables
that tell on the oracle alone what skipping a sample would leave in the output."""
import numpy as np

import fix2_cases as X
import flat_cases as F
from k1_diet_cases import band_aliased

REACH = 32
L = 17
SA, SB, SC, SD = 27, 18, 12, 8         # mulut_core.h kTubeSA .. kTubeSD


def tube_contains(a, b, c, d):
    """mulut_core.h tube_contains: the row's four keys span at most two steps"""
    mx, mn = np.maximum(np.maximum(a, b), np.maximum(c, d)), np.minimum(np.minimum(a, b), np.minimum(c, d))
    return mx - mn <= 2


def tube_slot(a, b, c, d):
    """mulut_core.h tube_slot"""
    return SA * a + SB * b + SC * c + SD * d


def _shifted(v, dy, dx, ylo, yhi):
    """v[clamp(y + dy, ylo, yhi)][clamp(x + dx, 0, W - 1)]: the kernels' clamps on a launch that may read rows ylo .. yhi"""
    H, W = v.shape[:2]
    ys = np.clip(np.arange(H) + dy, ylo, yhi)
    xs = np.clip(np.arange(W) + dx, 0, W - 1)
    return v[ys][:, xs]


def pass_ranges(img_hwc, modes, rows=None):
    """int16 [passes][H][W][C]: max - min of the four pixel values of every pass (mode of the sorted set of `modes` x rotation);
    rows = (oy0, oy1): neighbours clamped to rows oy0 - 2 .. oy1 + 1 of the frame, as a strip launch clamps them (the result is
    meaningful in rows oy0 .. oy1 - 1 only)."""
    v = np.asarray(img_hwc, np.uint8).astype(np.int16)
    H = v.shape[0]
    ylo, yhi = (0, H - 1) if rows is None else (max(rows[0] - F.HALO, 0), min(rows[1] + F.HALO, H) - 1)
    out = []
    for m in sorted(set(modes)):
        for r in range(4):
            vs = [v] + [_shifted(v, *F._rot(r, di, dj), ylo, yhi) for di, dj in F.PAT[m]]
            out.append(np.maximum.reduce(vs) - np.minimum.reduce(vs))
    return np.stack(out)


def far_mask(img_hwc, modes, rows=None):
    """bool [H][W][C]: some pass of the sample has values more than 32 levels apart (the fix-up kernel recomputes it when listed)"""
    return (pass_ranges(img_hwc, modes, rows) > REACH).any(0)


def flagged_mask(img_hwc, modes, rows=None):
    """bool [H][W][C]: what the tube kernels list (fix2_cases.dirty_mask, with a strip's row clamps when `rows` is given)"""
    if rows is None:
        return X.dirty_mask(img_hwc, modes)
    h = (np.asarray(img_hwc, np.uint8) >> 4).astype(np.int16)
    H = h.shape[0]
    ylo, yhi = max(rows[0] - F.HALO, 0), min(rows[1] + F.HALO, H) - 1
    out = np.zeros(h.shape, bool)
    for m in sorted(set(modes)):
        for r in range(4):
            hs = [h] + [_shifted(h, *F._rot(r, di, dj), ylo, yhi) for di, dj in F.PAT[m]]
            out |= (np.maximum.reduce(hs) - np.minimum.reduce(hs)) > 1
    return out


# ---------------------------------------------------------------------------------------------
# frames: four bands of rows
#   ramps   triangle waves of slope (kx, ky) per pixel, 6 .. 15 levels along an axis and 2 (kx + ky) <= 32: the passes of the d pattern
#           reach two pixels, so their values are up to 32 levels apart -- key MSBs two steps apart, every row still in the band
#   steps   plateaus four pixels wide that rise and fall by exactly 32 and exactly 33 levels in turn: the samples beside a step of 32
#           are flagged and skippable, the samples beside a step of 33 flagged and not
#   noise   uniform bytes: flagged, not skippable
#   smooth  one level per ~12 pixels: not flagged
# ---------------------------------------------------------------------------------------------
SLOPES = ((15, 0), (0, 15), (9, 6), (6, 10), (10, 6), (7, 8))


def _triangle(t, lo=8, hi=248):
    span = hi - lo
    t = np.mod(t, 2 * span)
    return lo + np.where(t > span, 2 * span - t, t)


def _plateaus(w, start):
    steps = (32, 33, 32, 33, 32, 33, -32, -33, -32, -33, -32, -33)
    levels = start + np.concatenate([[0], np.cumsum([steps[k % len(steps)] for k in range(w // 4 + 1)])])
    return np.repeat(levels, 4)[:w]


def frames(n, h, w, c, seed=0):
    """uint8 [n][h][w][c]"""
    rng = np.random.default_rng([seed, n, h, w, c])
    r0, r1, r2 = h // 3, (2 * h) // 3, (17 * h) // 20
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w, c), np.uint8)
    for f in range(n):
        for ch in range(c):
            kx, ky = SLOPES[(2 * f + ch) % len(SLOPES)]
            img = _triangle(kx * xx + ky * yy + 37 * ch + 11 * f)
            img[r0:r1] = _plateaus(w, 20 + 3 * ch + 7 * f)[None, :]
            img[r1:r2] = rng.integers(0, 256, (r2 - r1, w))
            img[r2:] = (100 + 20 * ch + (xx[r2:] + 2 * yy[r2:]) // 12)
            out[f, :, :, ch] = img.astype(np.uint8)
    return out


# the sizes of the existing fix-up tests, and one whose planar rows are whole dwords
SHAPES = ((X.N, X.H, X.W), (1, 40, 131), (X.N, X.H, 40))


def census(img_hwc, modes, rows=None):
    """(flagged and skippable, flagged and not skippable) sample counts of a frame (of its rows oy0 .. oy1 - 1 when `rows` is given)"""
    fl, far = flagged_mask(img_hwc, modes, rows), far_mask(img_hwc, modes, rows)
    if rows is not None:
        fl, far = fl[rows[0]:rows[1]], far[rows[0]:rows[1]]
    return int((fl & ~far).sum()), int((fl & far).sum())


def aliased(tables, fill):
    """What a tube kernel computes with when it flags nothing: every row outside the band replaced by whatever sits at its slot"""
    return [band_aliased(t, fill) for t in tables]


def identity_first_tables(modes):
    """First-stage tables whose cascade output is (nearly) the input: row (A, B, C, D) = 16 A - 127, so a stage gives the anchor's value
    back (the top level clips).  The strips of a pipeline then see the crafted frame as the final stage's input."""
    a = np.indices((L, L, L, L))[0].reshape(-1, 1)
    return {"s1_%s" % m: np.clip(16 * a - 127, -128, 127).astype(np.int8) for m in sorted(set(modes))}
