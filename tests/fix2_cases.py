"""Shared cases and NumPy reference of tests/test_fix2_cpu.py and tests/test_gpu_fix2.py (TEST ONLY; NumPy alone).

stage_up_fix2_kernel recomputes the samples the tube kernels put on their work list.  With the tube kernel on every tile
(final_stage_kernel = 5) and uniform-noise input nearly every sample is on the list, so the output is the fix-up kernel's product;
the list's length must then be the reference's number of dirty samples: a sample is dirty when one of its passes (a mode of the
list x a rotation) has four key MSBs that span more than one step (flat_cases.dirty_mask, here for any list of s, d, y)."""
import numpy as np

import flat_cases as F

# mode list -> table kinds it runs with.  sdys is M = 4: with the extreme tables its 16-bit fields reach the no-carry bound;
# sdysd is M = 5: the kernel's any-list body
LISTS = {"sdy": ("random",), "ysd": ("random",), "s": ("random",), "sd": ("random",), "sdys": ("random", "max", "min", "alt", "alt_c"),
         "sdysd": ("random",)}
N, H, W = 2, 21, 37            # W % 16 != 0, H % 4 != 0
STRIPS = ((0, 5), (5, 6), (6, 21))
POISON = 0xA5


def final_table(kind, mode, seed=0):
    """int8 [17^4][16]: seeded uniform noise, every value +127 / -128, or +127 / -128 alternating per element (alt_c: the complement)."""
    rows = 17 ** 4
    if kind == "random":
        return np.random.default_rng([seed, ord(mode), 16]).integers(-128, 128, (rows, 16)).astype(np.int8)
    if kind in ("max", "min"):
        return np.full((rows, 16), 127 if kind == "max" else -128, np.int8)
    even = (np.arange(16) % 2 == 0) != (kind == "alt_c")
    return np.broadcast_to(np.where(even, 127, -128).astype(np.int8), (rows, 16)).copy()


def luts(modes, kind, seed=0):
    """lut_dict of a two-stage x4 cascade: seeded random first-stage tables, final tables of `kind`."""
    out = {}
    for m in sorted(set(modes)):
        out["s1_%s" % m] = np.random.default_rng([seed, ord(m), 1]).integers(-128, 128, (17 ** 4, 1)).astype(np.int8)
        out["s2_%s" % m] = final_table(kind, m, seed)
    return out


def final_tables(lut_dict, modes):
    return [lut_dict["s2_%s" % m] for m in modes]


def first_tables(lut_dict, modes):
    return [lut_dict["s1_%s" % m] for m in modes]


def noise(n, h, w, c, seed=0):
    return np.random.default_rng([seed, n, h, w, c]).integers(0, 256, (n, h, w, c)).astype(np.uint8)


def dirty_mask(img_hwc, modes):
    """bool [H][W][C]: the sample has a pass of a mode of the list whose four key MSBs span more than one step."""
    h = (np.asarray(img_hwc, np.uint8) >> 4).astype(np.int16)
    out = np.zeros(h.shape, bool)
    for m in sorted(set(modes)):
        for r in range(4):
            hs = [h] + [F._shifted(h, *F._rot(r, di, dj)) for di, dj in F.PAT[m]]
            out |= (np.maximum.reduce(hs) - np.minimum.reduce(hs)) > 1
    return out


def ramp_and_noise(h=40, w=131, c=3, seed=3):
    """Left half a smooth ramp (one MSB step over ~40 pixels), right half uniform noise: smooth and detailed tiles in one frame."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.repeat((60 + 0.4 * xx + 0.3 * yy)[..., None], c, axis=2) + np.arange(c) * 5
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[:, w // 2:] = noise(1, h, w - w // 2, c, seed)[0]
    return img[None]


def step_edge(h=16, w=64, c=3):
    """A ramp inside one MSB level with one 48-level step between columns 40 and 41: a few dozen dirty samples beside the step."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = (96 + (xx % 8) + (yy % 4)).astype(np.uint8)
    img[:, 41:] += 48
    return np.repeat(img[..., None], c, axis=2)[None]


def constant(h=16, w=64, c=3, value=117):
    return np.full((1, h, w, c), value, np.uint8)


MANY = (8, 64, 256, 3)          # more samples than 8 x 256 CUs x 16 groups: every group walks the list past its first entry
GROUPS_PER_CU = 8 * 16

PAT = F.PAT                     # pattern offsets (di, dj) of keys b, c, d of a mode at rotation 0, as StageArgs::di / dj hold them
