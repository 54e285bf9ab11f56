"""Cases shared by test_val_cpu.py and test_gpu_val.py (GPU-free, seeded): the list of pairs the list scorer is held to
mulut_eval_y on, the inputs of mulut_ft_val_pack, a small validation folder, and the NumPy sums mulut_eval_finish turns into scores."""
import os

import numpy as np
from PIL import Image

import abi_sequences as A
from conftest import GOLDEN

# (name, H, W): one SSIM window (with shave 4 a 3 x 3 interior); one row of windows; exactly one 32 x 32 SSIM tile; four tiles, three
# of them one pixel thick; an odd size; 513 x 512 interior pixels with shave 4, just past the first grid-stride pass of 262,144
SHAPES = [("one_window", 11, 11), ("one_row", 11, 75), ("one_tile", 42, 42), ("four_tiles", 43, 43), ("odd", 53, 75),
          ("second_pass", 521, 520), ("identical", 53, 75), ("one_byte", 42, 42), ("noise", 53, 75)]
SHAVES = (2, 3, 4)


def list_pairs():
    """[(name, gt, out)] uint8 HWC RGB: natural-like frames against themselves plus rounding noise (as eval_pairs.py builds its pairs),
    an identical pair (PSNR inf), a pair that differs in one byte, and noise against noise."""
    from mulut_amd.synth import natural_frames
    rng = np.random.default_rng(77)
    pairs = []
    for k, (name, H, W) in enumerate(SHAPES):
        if name == "noise":
            gt, out = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        else:
            gt = natural_frames(1, H, W, 3, seed=100 + k)[0]
            out = np.clip(np.round(gt + rng.normal(0, 7, gt.shape)), 0, 255).astype(np.uint8)
            if name == "identical":
                out = gt.copy()
            elif name == "one_byte":
                out = gt.copy()
                out[20, 21, 1] ^= 0x10
        pairs.append((name, gt, out))
    return pairs


def pack_pools(pairs, order=None, gap=1):
    """(gt_pool, out_pool, rows): the pairs back to back in two byte pools, in `order`, `gap` bytes in front of each image of the
    ground-truth pool and 2 * gap + 1 in front of each of the output pool (so with gap 1 every offset but the first few is odd in one
    pool or the other, and the two differ); rows[i] = (gt_off, out_off, H, W) of item i of the plan."""
    order = list(range(len(pairs))) if order is None else order
    g, o, rows = [], [], []
    g_at = o_at = 0
    for i in order:
        _, gt, out = pairs[i]
        g.append(np.full(gap, 0xA5, np.uint8))
        o.append(np.full(2 * gap + 1, 0x5A, np.uint8))
        g_at, o_at = g_at + gap, o_at + 2 * gap + 1
        rows.append((g_at, o_at, gt.shape[0], gt.shape[1]))
        g.append(gt.reshape(-1))
        o.append(out.reshape(-1))
        g_at, o_at = g_at + gt.size, o_at + out.size
    return np.concatenate(g), np.concatenate(o), rows


def item_table(rows, gt_bytes, out_bytes):
    """mulut_eval_item[n] as an int64 [n][5] array: gt_off, out_off, (H, W) as two int32, the two pool sizes."""
    t = np.zeros((len(rows), 5), np.int64)
    for k, (g, o, H, W) in enumerate(rows):
        t[k, 0], t[k, 1], t[k, 3], t[k, 4] = g, o, gt_bytes, out_bytes
        t[k, 2:3].view(np.int32)[:] = (H, W)
    return t


def numpy_sums(gt, out, shave):
    """(sse, ssim_sum) of a pair as mulut_eval_plan_run defines them, in NumPy: the float32 squares of the float32 Y difference over
    the shaved interior added in float64, and the 'valid' SSIM map of common/utils.py:75-101 added up."""
    from scipy import signal
    from mulut_amd.metrics import _gaussian_kernel, rgb2ycbcr
    a, b = rgb2ycbcr(gt)[:, :, 0], rgb2ycbcr(out)[:, :, 0]
    d = (b.astype(np.float32) - a.astype(np.float32))[shave:-shave, shave:-shave]
    sse = float(np.sum(np.power(d, 2), dtype=np.float64))
    kx = _gaussian_kernel()
    window = kx * kx.T
    conv = lambda z: signal.convolve2d(z, window, "valid")  # noqa: E731
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return sse, float(np.sum(m))


# ------------------------------------------------------------------------------------------------------------ mulut_ft_val_pack
def pack_inputs():
    """{name: float32 [3][H][W]}: k / 255 for all 256 bytes on a 16 x 16 plane (the division the module's input went through, three
    planes rotated against each other); values on and beside every x.5 / 255 tie; values below 0 and above 1; small odd shapes."""
    k = np.arange(256, dtype=np.float32)
    bytes_ = (k / np.float32(255.0)).reshape(16, 16)
    t = ((np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255.0))
    lo, hi = np.float32(-1), np.float32(2)
    # [9][255]: the float32 next to (x + 0.5) / 255 and four neighbours on either side -- for every x the product of at least one of
    # them with 255.0f is x.5 exactly (a tie: round half to even), the others fall just below or above it
    rows, a, b = [t], t, t
    for _ in range(4):
        a, b = np.nextafter(a, lo), np.nextafter(b, hi)
        rows += [a, b]
    ties = np.stack(rows)
    assert ((ties * np.float32(255.0)) == (np.arange(255, dtype=np.float32) + np.float32(0.5))).any(axis=0).all()
    rng = np.random.default_rng(5)
    wide = rng.uniform(-0.5, 1.5, (3, 12, 13)).astype(np.float32)
    wide[0, 0, :6] = [-0.0, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), -1e-8, 255.4999 / 255]
    wide[1, 0, :4] = [np.inf, -np.inf, 1e30, -1e30]
    return {
        "bytes_16x16": np.stack([bytes_, np.roll(bytes_, 5, 1), bytes_.T.copy()]),
        "ties_9x255": np.stack([ties, ties[::-1].copy(), np.roll(ties, 1, 0)]),
        "out_of_range_12x13": wide,
        "one_pixel": np.array([0.2, 0.5, 0.9], np.float32).reshape(3, 1, 1),
        "odd_3x5": rng.uniform(0, 1, (3, 3, 5)).astype(np.float32),
    }


# ------------------------------------------------------------------------------------------------------------ a validation folder
def write_val_dir(root, scale=4):
    """{root}/{Set5, Set14}/{HR, LR_bicubic/X4}: five pairs with LR sizes around 20 x 24 in two datasets, one of them grey and one
    whose HR is no multiple of the scale in either dimension (LR: the modcropped size / scale).  Stems with a '_': the reference names
    a result after the last '_'-token.  Returns (root, {dataset: sorted file names})."""
    from mulut_amd.synth import natural_frames
    s, files = scale, {}

    def put(ds, name, hr, extra=(0, 0)):
        hr_dir, lr_dir = os.path.join(str(root), ds, "HR"), os.path.join(str(root), ds, "LR_bicubic", "X%d" % s)
        os.makedirs(hr_dir, exist_ok=True)
        os.makedirs(lr_dir, exist_ok=True)
        Image.fromarray(hr).save(os.path.join(hr_dir, name))
        H, W = hr.shape[0] - extra[0], hr.shape[1] - extra[1]
        core = hr[:H, :W].reshape((H // s, s, W // s, s) + hr.shape[2:])
        Image.fromarray(core.mean(axis=(1, 3)).round().astype(np.uint8)).save(os.path.join(lr_dir, name))
        files.setdefault(ds, []).append(name)

    put("Set5", "img_001.png", natural_frames(1, 20 * s, 24 * s, 3, seed=71)[0])
    put("Set5", "img_002.png", natural_frames(1, 24 * s, 20 * s, 3, seed=72)[0])
    put("Set5", "plain.png", natural_frames(1, 22 * s, 26 * s, 3, seed=73)[0])
    put("Set14", "zz_grey.png", natural_frames(1, 21 * s, 23 * s, 1, seed=74)[0, :, :, 0])
    put("Set14", "zz_odd.png", natural_frames(1, 19 * s + 2, 25 * s + 3, 3, seed=75)[0], extra=(2, 3))
    return str(root), {ds: sorted(v) for ds, v in files.items()}


def write_exp(folder, modes, interval, shipped):
    """The transferred tables a fine-tune run starts from, 2 stages x4: the shipped LUT_ft tables (s, d, y at interval 4) or smooth
    make_table tables."""
    os.makedirs(str(folder), exist_ok=True)
    for s in (1, 2):
        for m in modes:
            if shipped:
                t = np.load(os.path.join(GOLDEN, "luts", "LUT_ft_x4_4bit_int8_s%d_%s.npy" % (s, m)))
            else:
                t = A.make_table(np.random.default_rng(10 * s + ord(m)), interval, 16 if s == 2 else 1, True)
            np.save(os.path.join(str(folder), "LUT_x4_%dbit_int8_s%d_%s.npy" % (interval, s, m)), t)
    return str(folder)


MODELS = [("MuLUT", "sdy", 4, True), ("MuLUTInterval", "sdy", 5, False), ("MuLUTWide", "eho", 4, False)]
