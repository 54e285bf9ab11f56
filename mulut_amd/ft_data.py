"""The training set of the fine-tune driver (mulut_amd/finetune_lut.py): the scan of ``{trainDir}``, the draw of one sample, and the two
providers that cut batches from them -- ``CropProvider`` on the host (the reference's path, sr/data.py:96-124) and
``DeviceCropProvider`` on the device (``mulut_ft_crop_batch``).  Both take their pairs from ``scan_pairs`` and their draws from
``draw_sample``, so the same ``--seed`` gives the same batches, bit for bit, by construction."""
import os
import random

import numpy as np
import torch
from PIL import Image

from . import _native
from .resample import bicubic, resize_image


class _PendingLR:
    """An LR image that DeviceCropProvider will have the resample kernel write straight into its pool slot: only its shape."""
    dtype = np.dtype(np.uint8)

    def __init__(self, shape):
        self.shape, self.size = tuple(shape), int(np.prod(shape))


def scan_pairs(path, scale, patch, make_lr=False, log=print, defer=False):
    """The training pairs [(lr, hr)] as H x W x C arrays, in sorted order of ``{path}/HR``: the LR twin is ``LR/X{scale}/<stem>x{scale}.png``
    (DIV2K layout) or ``LR_bicubic/X{scale}/<stem>.png`` (benchmark layout); a pair whose LR is smaller than the patch is left out.
    `make_lr`: an HR file without a twin gets the (w // s, h // s) bicubic image of sr/Test_dataset.py:24-25 (no modcrop) -- modes L
    and RGB on the device, or with `defer` as a _PendingLR for the caller to make; any other mode through Pillow, with one log line."""
    hr_dir = os.path.join(path, "HR")
    pairs = []
    for fn in sorted(os.listdir(hr_dir)):
        for lr in (os.path.join(path, "LR", "X%d" % scale, "%sx%d.png" % (fn[:-4], scale)),
                   os.path.join(path, "LR_bicubic", "X%d" % scale, fn)):
            if os.path.exists(lr):
                hr_im = np.array(Image.open(os.path.join(hr_dir, fn)))
                lr_im = np.array(Image.open(lr))
                if hr_im.ndim == 2:
                    hr_im, lr_im = hr_im[:, :, None], lr_im[:, :, None]
                if min(lr_im.shape[:2]) >= patch:
                    pairs.append((lr_im, hr_im))
                break
        else:
            if make_lr:
                pairs.extend(_made_pair(Image.open(os.path.join(hr_dir, fn)), fn, scale, patch, log, defer))
    if not pairs:
        raise FileNotFoundError("no HR/LR training pairs with LR >= %d px under %s" % (patch, path))
    return pairs


def _made_pair(img, fn, s, patch, log, defer):
    h, w = img.height // s, img.width // s
    if min(h, w) < max(patch, 1):
        return []
    hr_im = np.array(img)
    if img.mode in ("L", "RGB"):
        if hr_im.ndim == 2:
            hr_im = hr_im[:, :, None]
        lr_im = _PendingLR((h, w, hr_im.shape[2])) if defer else bicubic(hr_im, (h, w))
    else:                                  # Pillow on the host, one log line
        lr_im = np.array(resize_image(img, (w, h), log, fn))
        if hr_im.ndim == 2:
            hr_im, lr_im = hr_im[:, :, None], lr_im[:, :, None]
    return [(lr_im, hr_im)]


_TURNS = [0, 1, 2, 3]


def draw_sample(rng, shapes, sz):
    """One training sample (pair, i, j, c, flips, k) from `rng` (a random.Random), in the reference's order (sr/data.py:96-124): the pair,
    the patch's row and column in the LR image, the channel, flip left-right (bit 0 of flips), flip up-down (bit 1), quarter turns.
    `shapes`: (lr_h, lr_w, ch) per pair; `sz`: the LR patch size.  This is the only place that decides how a batch consumes the seed."""
    n = rng.choice(range(len(shapes)))
    h, w, ch = shapes[n]
    i = rng.randint(0, h - sz)
    j = rng.randint(0, w - sz)
    c = rng.randrange(ch)
    lr = rng.uniform(0, 1) < 0.5
    ud = rng.uniform(0, 1) < 0.5
    return n, i, j, c, lr + 2 * ud, rng.choice(_TURNS)


class CropProvider:
    """Random (LR crop, HR crop) batches, one colour channel each, flips + rot90 as sr/data.py:96-124.  `pairs`: a scan already made
    (scan_pairs' list, nothing pending) instead of one of `path`."""

    def __init__(self, path, scale, patch, batch, seed=None, make_lr=False, log=print, pairs=None):
        self.scale, self.sz, self.batch = scale, patch, batch
        self.rng = random.Random(seed)
        self.pairs = scan_pairs(path, scale, patch, make_lr, log) if pairs is None else pairs
        self.shapes = [lr_im.shape for lr_im, _ in self.pairs]

    def next(self):
        ims, lbs, s, sz = [], [], self.scale, self.sz
        for _ in range(self.batch):
            n, i, j, c, flips, k = draw_sample(self.rng, self.shapes, sz)
            im, lb = self.pairs[n]
            lb = lb[i * s:(i + sz) * s, j * s:(j + sz) * s, c]
            im = im[i:i + sz, j:j + sz, c]
            if flips & 1:
                lb, im = np.fliplr(lb), np.fliplr(im)
            if flips & 2:
                lb, im = np.flipud(lb), np.flipud(im)
            lbs.append(np.rot90(lb, k).astype(np.float32)[None] / 255.0)
            ims.append(np.rot90(im, k).astype(np.float32)[None] / 255.0)
        return torch.from_numpy(np.stack(ims)).cuda(), torch.from_numpy(np.stack(lbs)).cuda()


class TrainingSetTooLarge(Exception):
    """The packed training set is larger than the caller allows on the device; ``host`` is the loaded CropProvider (same seed, no
    draw taken yet) to go on with."""

    def __init__(self, nbytes, limit, host):
        super().__init__("training set of %d bytes exceeds the %d allowed on the device" % (nbytes, limit))
        self.nbytes, self.limit, self.host = nbytes, limit, host


class DeviceCropProvider:
    """CropProvider's batches, bit for bit for the same seed, cut on the device (mulut_ft_crop_batch): the pairs of scan_pairs, in its
    order, lie in one uint8 device tensor as the PNGs decode; next() takes the batch's draws from draw_sample, sends those B x 6
    integers through a ring of pinned buffers and launches once on the current stream.  next() never waits for the device unless
    the host is RING batches ahead of it: a slot's event, recorded behind its copy, is waited for before the slot is rewritten."""
    RING = 32

    def __init__(self, path, scale, patch, batch, seed=None, max_bytes=None, make_lr=False, log=print):
        pairs = scan_pairs(path, scale, patch, make_lr, log, defer=True)
        self.scale, self.sz, self.batch = scale, patch, batch
        self.rng = random.Random(seed)
        table, off = np.zeros((len(pairs), 10), np.int32), 0
        t64 = table.view(np.int64)                                 # mulut_ft_pair: two 64-bit offsets, then lr_h, lr_w, hr_h, hr_w, ch, pad
        for n, (lr_im, hr_im) in enumerate(pairs):
            if lr_im.dtype != np.uint8 or hr_im.dtype != np.uint8 or lr_im.shape[2] != hr_im.shape[2]:
                raise ValueError("pair %d is not a pair of 8-bit images with the same channels (--hostData takes it)" % n)
            t64[n, 0], t64[n, 1] = off, off + lr_im.size
            table[n, 4:9] = lr_im.shape[0], lr_im.shape[1], hr_im.shape[0], hr_im.shape[1], lr_im.shape[2]
            off += lr_im.size + hr_im.size
        self.pool_bytes = off
        if max_bytes is not None and off > max_bytes:              # the pending LR images made on the device and copied back
            pairs = [(bicubic(hr_im, lr_im.shape[:2]) if isinstance(lr_im, _PendingLR) else lr_im, hr_im) for lr_im, hr_im in pairs]
            raise TrainingSetTooLarge(off, max_bytes, CropProvider(path, scale, patch, batch, seed, pairs=pairs))
        self.shapes = [im.shape for im, _ in pairs]                # (lr_h, lr_w, ch) per pair: all the draws need
        self.device = torch.empty(0).cuda().device
        self.pool = torch.empty(off, dtype=torch.uint8, device=self.device)
        for n, (lr_im, hr_im) in enumerate(pairs):                 # image by image: no second copy of the set on the host
            a = int(t64[n, 0])
            hr_slot = self.pool[a + lr_im.size:a + lr_im.size + hr_im.size]
            hr_slot.copy_(torch.from_numpy(np.ascontiguousarray(hr_im).reshape(-1)))
            if isinstance(lr_im, _PendingLR):                      # --makeLR: the kernel writes the pair's LR slot from its HR slot
                bicubic(hr_slot.view(hr_im.shape), lr_im.shape[:2], out=self.pool[a:a + lr_im.size])
            else:
                self.pool[a:a + lr_im.size].copy_(torch.from_numpy(np.ascontiguousarray(lr_im).reshape(-1)))
        self.table = torch.from_numpy(table).cuda()
        self.bad = torch.zeros(1, dtype=torch.int32).cuda()         # samples the kernel refused: stays 0 (the draws are legal by construction)
        if self.pool.is_cuda:
            torch.cuda.synchronize(self.device)                    # the set is in place whatever stream next() is called on
        self._ring, self._events, self._slot, self._lib = None, None, 0, None

    def draw(self, out=None):
        """The host half of next(): the batch's draws as int32 [B][6] = pair, i, j, c, flips (bit 0 lr, bit 1 ud), k."""
        out = np.empty((self.batch, 6), np.int32) if out is None else out
        out[:] = [draw_sample(self.rng, self.shapes, self.sz) for _ in range(self.batch)]
        return out

    def next(self):
        if self._ring is None:
            self._lib = _native.load()
            self._ring = [torch.empty((self.batch, 6), dtype=torch.int32).pin_memory() for _ in range(self.RING)]
            self._events = [None] * self.RING
        slot, self._slot = self._slot, (self._slot + 1) % self.RING
        if self._events[slot] is not None:
            self._events[slot].synchronize()                       # (returns at once unless the host is RING batches ahead)
        else:
            self._events[slot] = torch.cuda.Event()
        self.draw(self._ring[slot].numpy())
        stream = torch.cuda.current_stream(self.device)
        draws = self._ring[slot].to(self.device, non_blocking=True)
        self._events[slot].record(stream)
        im = torch.empty((self.batch, 1, self.sz, self.sz), dtype=torch.float32, device=self.device)
        lb = torch.empty((self.batch, 1, self.sz * self.scale, self.sz * self.scale), dtype=torch.float32, device=self.device)
        _native.check(self._lib.mulut_ft_crop_batch(self.device.index, self.pool.data_ptr(), self.pool_bytes, self.table.data_ptr(), len(self.shapes),
                                                    draws.data_ptr(), self.batch, self.sz, self.scale, im.data_ptr(), lb.data_ptr(),
                                                    self.bad.data_ptr(), _native.stream_ptr(self.device)))
        return im, lb
