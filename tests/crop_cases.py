"""Shared by tests/test_crop_cpu.py and tests/test_gpu_crop.py: a small synthetic training set written as PNGs, and the crop of
sr/data.py:91-121 applied to a table of draws with np.fliplr / np.flipud / np.rot90 literally (the checker of mulut_ft_crop_batch)."""
import os

import numpy as np
from PIL import Image

SZ_MAX = 57      # the largest patch the tests cut: every pair's LR is at least this in both dimensions


def write_set(root, scale):
    """{root}/HR/<stem>.png with {root}/LR_bicubic/X{scale}/<stem>.png (benchmark layout; pair e in the DIV2K layout, LR/X{scale}/<stem>x{scale}.png):
      a_rgb     RGB, LR 57 x 86
      b_grey    grey ('L'), LR 60 x 59
      c_tight   RGB, LR exactly 57 rows (at sz = 57 only i = 0 is legal) x 70
      d_ragged  RGB, LR 58 x 61, HR 2 rows and 3 columns larger than scale * LR
      e_bytes   RGB, LR 64 x 64 holding all 256 byte values in every channel (HR: every value in every scale x scale block row)
    Returns the directory."""
    rng = np.random.default_rng(1234 + scale)
    root = str(root)
    os.makedirs(os.path.join(root, "HR"))
    os.makedirs(os.path.join(root, "LR_bicubic", "X%d" % scale))
    os.makedirs(os.path.join(root, "LR", "X%d" % scale))

    def put(stem, lr, hr, div2k=False):
        Image.fromarray(hr).save(os.path.join(root, "HR", stem + ".png"))
        Image.fromarray(lr).save(os.path.join(root, "LR", "X%d" % scale, "%sx%d.png" % (stem, scale)) if div2k
                                 else os.path.join(root, "LR_bicubic", "X%d" % scale, stem + ".png"))

    def noise(h, w, *c):
        return rng.integers(0, 256, (h, w) + c, dtype=np.uint8)

    put("a_rgb", noise(57, 86, 3), noise(57 * scale, 86 * scale, 3))
    put("b_grey", noise(60, 59), noise(60 * scale, 59 * scale))
    put("c_tight", noise(57, 70, 3), noise(57 * scale, 70 * scale, 3))
    put("d_ragged", noise(58, 61, 3), noise(58 * scale + 2, 61 * scale + 3, 3))
    ramp = (np.arange(64 * 64).reshape(64, 64) % 256).astype(np.uint8)
    lr = np.stack([ramp, ramp[::-1], ramp.T], 2)
    hr = np.stack([np.kron(lr[:, :, c], np.ones((scale, scale), np.uint8)) for c in range(3)], 2)
    hr = (hr.astype(np.int32) + np.arange(64 * scale)[None, :, None] * 37).astype(np.uint8)
    put("e_bytes", np.ascontiguousarray(lr), np.ascontiguousarray(hr), div2k=True)
    return root


def apply_draws(pairs, draws, sz, scale):
    """pairs: [(lr HWC uint8, hr HWC uint8)], draws: int [B][6] = pair, i, j, c, flips, k -> (im [B][1][sz][sz], lb [B][1][sz*s][sz*s]) float32,
    the statements of sr/data.py:101-119 one by one."""
    ims, lbs = [], []
    s = scale
    for n, i, j, c, flips, k in np.asarray(draws).tolist():
        im, lb = pairs[n]
        lb = lb[i * s:i * s + sz * s, j * s:j * s + sz * s, c]
        im = im[i:i + sz, j:j + sz, c]
        if flips & 1:
            lb, im = np.fliplr(lb), np.fliplr(im)
        if flips & 2:
            lb, im = np.flipud(lb), np.flipud(im)
        lb, im = np.rot90(lb, k), np.rot90(im, k)
        lbs.append(np.expand_dims(lb.astype(np.float32) / 255.0, axis=0))
        ims.append(np.expand_dims(im.astype(np.float32) / 255.0, axis=0))
    return np.stack(ims), np.stack(lbs)
