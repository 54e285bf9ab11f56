"""LR images made on the device: Pillow's bicubic resampling, byte for byte (the reference's sr/Test_dataset.py:14-27).

    python -m mulut_amd.resample <HR dir> <output root> [--scales 2 3 4] [--layout div2k|benchmark]

The reference makes ``LR/X{s}/<stem>x{s}.png`` from ``HR/<stem>.png`` with ``img.resize((w // s, h // s), resample=Image.BICUBIC)``
for s = 2, 3, 4.  ``bicubic`` runs that resize as one HIP launch (``mulut_resample_run``, mulut_amd/csrc/mulut_resample.hip) on uint8
device tensors, with the tables of a cached plan per size pair; ``make_lr`` is the script's loop over a folder, writing either the
script's names (``layout="div2k"``) or ``LR_bicubic/X{s}/<stem>.png`` (``layout="benchmark"``: what the test script and the fine-tune
validation read).  The same kernel run the other way is the bicubic upscaling every SR table starts from
(``python -m mulut_amd.test_lut --bicubicBaseline``).  There is no CPU path: without a GPU ``bicubic`` raises.
"""
import argparse
import ctypes
import os

import numpy as np
import torch
from PIL import Image

from . import _native
from .engine import MuLUTError

LAYOUT_CHW, LAYOUT_HWC = 0, 1
TILE_H, TILE_H_UP = 16, 64      # output rows of a workgroup's tile (kRsTileH), and where the image grows downwards (kRsTileHUp)
MAX_PLANS = 64       # cached plans; the least recently used one is destroyed beyond that

_plans = {}          # (device index, in_h, in_w, out_h, out_w) -> _Plan, in order of last use


def tile_w(channels=1, packed=True):
    """Output pixels across a tile of the kernel: 256 bytes of a row, whole pixels and whole dwords of it (252 bytes at C = 3), when
    both images are HWC with at most 4 channels; 256 pixels of one channel for any other layout or C."""
    c = int(channels) if packed and channels <= 4 else 1
    return 256 // (4 * c) * 4


def coeffs(in_size, out_size):
    """One axis' tables as Pillow builds them (host only): (kk int32 [out][taps], xmin int32 [out], n int32 [out])."""
    lib = _native.load()
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be positive")
    taps = 2 * int(np.ceil(2.0 * max(in_size / out_size, 1.0))) + 1
    kk = np.zeros((out_size, taps), np.int32)
    xmin, n = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    got = _native.check(lib.mulut_resample_coeffs(in_size, out_size, kk.ctypes.data_as(i32p), xmin.ctypes.data_as(i32p), n.ctypes.data_as(i32p), kk.size),
                        MuLUTError)
    assert got == taps
    return kk, xmin, n


class _Plan:
    def __init__(self, lib, device, in_h, in_w, out_h, out_w):
        self._lib, self._h = lib, ctypes.c_void_p()
        _native.check(lib.mulut_resample_plan_create(device, in_h, in_w, out_h, out_w, ctypes.byref(self._h)), MuLUTError)

    def close(self):
        if self._h:
            self._lib.mulut_resample_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _plan(device, in_h, in_w, out_h, out_w):
    key = (device, in_h, in_w, out_h, out_w)
    plan = _plans.pop(key, None)
    if plan is None:
        plan = _Plan(_native.load(), *key)
        while len(_plans) >= MAX_PLANS:
            _plans.pop(next(iter(_plans))).close()
    _plans[key] = plan
    return plan


def clear_plans():
    while _plans:
        _plans.popitem()[1].close()


def bicubic(x, size, out=None):
    """``Image.fromarray(x).resize((size[1], size[0]), Image.BICUBIC)`` on the device.

    x: uint8, HW (grey), HWC, or NCHW -- a device tensor, or a host tensor / NumPy array (copied to cuda:0 and back; a NumPy array in
    gives a NumPy array out).  size: (out_h, out_w).  out: optional uint8 device tensor of the result's size to write into (same
    layout as x), e.g. a slice of a larger buffer.  Runs on the current stream of x's device and does not wait for it."""
    lib = _native.load()
    if not torch.cuda.is_available():
        raise MuLUTError("no GPU visible: mulut_amd has no CPU path")
    as_numpy = isinstance(x, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(x)) if as_numpy else x
    if t.dtype != torch.uint8:
        raise TypeError("bicubic wants uint8, got %s" % (t.dtype,))
    on_host = not t.is_cuda
    t = (t.cuda() if on_host else t).contiguous()
    out_h, out_w = int(size[0]), int(size[1])
    if t.dim() == 2:
        N, C, (in_h, in_w), layout, shape = 1, 1, t.shape, LAYOUT_HWC, (out_h, out_w)
    elif t.dim() == 3:
        N, (in_h, in_w, C), layout = 1, t.shape, LAYOUT_HWC
        shape = (out_h, out_w, C)
    elif t.dim() == 4:
        (N, C, in_h, in_w), layout = t.shape, LAYOUT_CHW
        shape = (N, C, out_h, out_w)
    else:
        raise ValueError("bicubic wants HW, HWC or NCHW, got %d dimensions" % t.dim())
    if min(N, C, in_h, in_w, out_h, out_w) < 1:
        raise ValueError("empty image or size")
    if out is None:
        res = torch.empty(shape, dtype=torch.uint8, device=t.device)
    else:
        res = out
        if not res.is_cuda or res.device != t.device or res.dtype != torch.uint8 or not res.is_contiguous() or res.numel() != N * C * out_h * out_w:
            raise ValueError("out must be a contiguous uint8 tensor of %d elements on %s" % (N * C * out_h * out_w, t.device))
    plan = _plan(t.device.index, int(in_h), int(in_w), out_h, out_w)
    with torch.cuda.device(t.device):
        _native.check(lib.mulut_resample_run(plan._h, t.data_ptr(), layout, res.data_ptr(), layout, int(N), int(C), _native.stream_ptr(t.device)),
                      MuLUTError)
    if out is not None:
        return out
    if as_numpy:
        return res.cpu().numpy()
    return res.cpu() if on_host else res


def resize_image(img, size, log=print, name=""):
    """A PIL image resized to size = (width, height) like ``img.resize(size, Image.BICUBIC)``: modes L and RGB on the device; any
    other mode (palette, 1-bit, 16-bit, LA / RGBA which Pillow premultiplies, ...) through Pillow on the host, with one log line."""
    if img.mode in ("L", "RGB"):
        return Image.fromarray(bicubic(np.array(img), (size[1], size[0])))
    log("{}: mode {} is resized by Pillow on the host".format(name or "image", img.mode))
    return img.resize(size, resample=Image.BICUBIC)


def lr_path(out_root, stem, scale, layout):
    if layout == "div2k":
        return os.path.join(out_root, "LR", "X%d" % scale, "%sx%d.png" % (stem, scale))      # sr/Test_dataset.py:26
    if layout == "benchmark":
        return os.path.join(out_root, "LR_bicubic", "X%d" % scale, "%s.png" % stem)          # sr/4_test_lut.py:265
    raise ValueError("layout must be 'div2k' or 'benchmark', got %r" % (layout,))


def make_lr(hr_dir, out_root, scales=(2, 3, 4), layout="div2k", log=print):
    """sr/Test_dataset.py:14-27 for every ``*.png`` of hr_dir: the (w // s, h // s) bicubic image per scale, saved as PNG under
    out_root in the reference script's names (layout "div2k") or the benchmark folders' (layout "benchmark").  Returns the paths."""
    for s in scales:
        os.makedirs(os.path.dirname(lr_path(out_root, "x", s, layout)), exist_ok=True)      # :15-16
    written = []
    for fn in sorted(os.listdir(hr_dir)):
        if not fn.lower().endswith(".png"):
            continue
        img = Image.open(os.path.join(hr_dir, fn))
        stem = os.path.splitext(fn)[0]
        for s in scales:
            new_size = (img.width // s, img.height // s)
            if min(new_size) < 1:
                raise ValueError("%s is smaller than the scale %d" % (fn, s))
            path = lr_path(out_root, stem, s, layout)
            resize_image(img, new_size, log, fn).save(path)
            written.append(path)
    log("{} LR images written under {}".format(len(written), out_root))
    return written


def bicubic_baseline(run):
    """The first column of an SR table for one dataset of the test script: every LR image of `run` (a ``mulut_amd.test_lut.eltr``)
    upscaled x scale by Pillow's bicubic filter on the device and scored like a result of the cascade -- ``engine.eval_y`` with
    device metrics, the host metrics of ``eltr._finish`` without.  Prints one line and returns float64 [images][2]."""
    from .metrics import psnr, rgb2ycbcr, ssim
    s, scores = run.opt.scale, []
    for i in range(len(run.files)):
        img_lr, img_gt = run._load(i)
        if img_lr.ndim == 2:
            img_lr = np.stack([img_lr] * 3, axis=2)
        x = torch.from_numpy(np.ascontiguousarray(img_lr)).to(run.engine.device)
        up = bicubic(x, (img_lr.shape[0] * s, img_lr.shape[1] * s))
        if run.device_metrics:
            gt = torch.from_numpy(np.ascontiguousarray(img_gt)).to(run.engine.device)
            scores.append(list(run.engine.eval_y(gt, up, s)))
        else:
            y_gt, y_out = rgb2ycbcr(img_gt)[:, :, 0], rgb2ycbcr(up.cpu().numpy())[:, :, 0]
            scores.append([psnr(y_gt, y_out, s), ssim(y_gt, y_out)])
    arr = np.asarray(scores)
    print('Dataset {} | AVG Bicubic PSNR: {:.2f} SSIM: {:.4f}'.format(run.dataset, np.mean(arr[:, 0]), np.mean(arr[:, 1])))
    return arr


def add_baseline_line(eltr):
    """``--bicubicBaseline`` (mulut_amd/options.py): wrap ``eltr.run`` once, so that an evaluator whose options carry the flag prints
    the baseline line behind its summary and keeps the scores as ``.baseline``.  Evaluators without the flag run as before."""
    if getattr(eltr.run, "_with_baseline", False):
        return
    plain = eltr.run

    def run(self, *args, **kwargs):
        arr = plain(self, *args, **kwargs)
        if getattr(self.opt, "bicubicBaseline", False):
            self.baseline = bicubic_baseline(self)
        return arr

    run._with_baseline = True
    run.__doc__ = plain.__doc__
    eltr.run = run


def main(argv=None):
    p = argparse.ArgumentParser(description="Make bicubic LR images from a folder of HR images on the GPU (Pillow's bytes).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("hr_dir", help="folder of HR *.png (the reference script's hr_path)")
    p.add_argument("out_root", help="root that receives LR/X{s}/ or LR_bicubic/X{s}/ (the reference script's lr_base_path is {out_root}/LR)")
    p.add_argument("--scales", type=int, nargs="+", default=[2, 3, 4])
    p.add_argument("--layout", choices=["div2k", "benchmark"], default="div2k",
                   help="div2k: LR/X{s}/<stem>x{s}.png (the reference script's names); benchmark: LR_bicubic/X{s}/<stem>.png")
    opt = p.parse_args(argv)
    return make_lr(opt.hr_dir, opt.out_root, tuple(opt.scales), opt.layout)


if __name__ == "__main__":
    main()
