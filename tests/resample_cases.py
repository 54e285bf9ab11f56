"""Shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py: Pillow's 8-bit bicubic resize restated in NumPy
(precompute_coeffs, normalize_coeffs_8bpc and the two 8bpc passes of Pillow's Resample.c, vectorised over the output positions with
every double operation in Pillow's order), the case list, and Pillow itself as the judge."""
import numpy as np
from PIL import Image

PRECISION = 22
SIZES = [(1, 9), (4, 4), (5, 7), (9, 4), (37, 53), (48, 48), (64, 65), (17, 301), (255, 3), (130, 258)]      # (h, w)
CONTENTS = ("noise", "ends", "ramp")
SCALES = (2, 3, 4)
PAIRS = [(2040, 510), (2041, 510), (1356, 339), (1080, 4320)]


def bic(x, a=-0.5):
    x = np.abs(x)
    with np.errstate(all="ignore"):
        return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def coeffs(insz, outsz):
    """(kk int32 [out][taps], zero beyond a row's n; xmin int32 [out]; n int32 [out]) for one axis."""
    scale = insz / outsz
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(outsz) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), insz)
    n = xmax - xmin
    k = np.zeros((outsz, ksize))
    ww = np.zeros(outsz)
    for x in range(ksize):                       # the sum runs in index order
        w = np.where(x < n, bic((x + xmin - center + 0.5) * ss), 0.0)
        k[:, x] = w
        ww = np.where(x < n, ww + w, ww)
    k = np.where((ww != 0.0)[:, None], k / np.where(ww != 0.0, ww, 1.0)[:, None], k)
    kk = np.where(k < 0, -0.5 + k * (1 << PRECISION), 0.5 + k * (1 << PRECISION)).astype(np.int64)      # (int): towards zero
    kk[np.arange(ksize)[None, :] >= n[:, None]] = 0
    return kk.astype(np.int32), xmin.astype(np.int32), n.astype(np.int32)


def pass1(a, outsz):
    """One pass along axis 1 of a uint8 array, into rounded and clipped uint8."""
    kk, xm, cnt = coeffs(a.shape[1], outsz)
    out = np.empty((a.shape[0], outsz) + a.shape[2:], np.uint8)
    a = a.astype(np.int64)
    for xx in range(outsz):
        s = np.full((a.shape[0],) + a.shape[2:], 1 << (PRECISION - 1), np.int64)
        for x in range(cnt[xx]):
            s += a[:, xm[xx] + x] * int(kk[xx, x])
        assert np.abs(s).max() < 2 ** 31          # an int32 accumulator is exact
        out[:, xx] = np.clip(s >> PRECISION, 0, 255)
    return out


def resize(a, out_h, out_w):
    """a: uint8 HW or HWC.  The horizontal pass, then the vertical pass over its bytes; an unchanged axis is skipped."""
    if out_w != a.shape[1]:
        a = pass1(a, out_w)
    if out_h != a.shape[0]:
        a = pass1(a.swapaxes(0, 1), out_h).swapaxes(0, 1)
    return np.ascontiguousarray(a)


def pil_resize(a, out_h, out_w):
    return np.array(Image.fromarray(a).resize((out_w, out_h), resample=Image.BICUBIC))


def image(h, w, kind, channels, seed=0):
    """uint8 [h][w][channels] ([h][w] for channels = 0, mode L).  'ends' holds only 0 and 255: the negative lobes reach both clips."""
    c = max(channels, 1)
    rng = np.random.default_rng([seed, h, w, c])
    a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "ends":
        a = (a > 127).astype(np.uint8) * 255
    elif kind == "ramp":
        a = ((np.arange(h)[:, None, None] * 7 + np.arange(w)[None, :, None] * 5 + np.arange(c) * 40) % 256).astype(np.uint8)
    else:
        assert kind == "noise"
    return np.ascontiguousarray(a if channels else a[:, :, 0])


def cases():
    """(h, w, kind, channels, out_h, out_w): every size x content x factor (/2 /3 /4 x2 x3 x4) x mode (L: channels 0, RGB: 3)."""
    out = []
    for h, w in SIZES:
        for kind in CONTENTS:
            for ch in (0, 3):
                for s in SCALES:
                    if h // s and w // s:
                        out.append((h, w, kind, ch, h // s, w // s))
                    out.append((h, w, kind, ch, h * s, w * s))
    return out
