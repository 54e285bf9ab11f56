"""GPU twin of the reference's LUT fine-tuning driver (sr/3_finetune_lut.py:68-172).

    python -m mulut_amd.finetune_lut --stages 2 --modes sdy -e <expDir> --trainDir <DIV2K-like dir> [--totalIter 2000]

Reads the transferred tables ``LUT_x{scale}_{interval}bit_int8_s{stage}_{mode}.npy`` from expDir (sr/model.py:51-53),
optimises them with Adam + the reference's cosine LambdaLR on random single-channel crops with the reference's
rigid augmentation (sr/data.py:96-124), and writes ``LUT_ft_x{scale}_{interval}bit_int8_s{stage}_{mode}.npy``
(sr/3_finetune_lut.py:162-169).  The model is ``mulut_amd.finetune.MuLUT``, at ``--interval 5`` / ``6`` ``MuLUTInterval``, and ``MuLUTWide`` at any of the three
intervals when ``--modes`` holds one of the 4 x 4 patterns e, h, o (HIP forward/backward kernels).
Training pairs: ``{trainDir}/HR/<stem>.png`` with ``{trainDir}/LR/X{scale}/<stem>x{scale}.png`` (DIV2K layout) or
``{trainDir}/LR_bicubic/X{scale}/<stem>.png`` (benchmark layout).  ``valid_steps`` is the reference's validation loop
(:23-65): every ``--valStep`` iterations (and at iteration 1) each benchmark image goes through the module, the result is
saved as ``{valoutDir}/{dataset}/{last '_'-token of the stem}_lutft.png`` (the reference's naming) and Y-PSNR / SSIM are averaged per dataset -- computed on the device
(``mulut_eval_y``), logged with the reference's line.

Training batches come from ``DeviceCropProvider``: the pairs lie on the device as the uint8 bytes the PNGs hold and one HIP launch
(``mulut_ft_crop_batch``) cuts, flips, turns and converts a batch from six host-drawn integers per sample -- the same batches, bit for
bit, as ``CropProvider`` (the reference's host path, kept as ``--hostData`` and as the fallback when the set does not fit the device)
gives for the same ``--seed``.  The loop does not wait for the device per step: losses go into a device vector that is read every
``--displayStep`` iterations, so the logged ``rT`` is WALL time per iteration between two display points (data, step and the read-back
included), not the reference's host-side time of the step alone.

``--makeLR``: an HR file without an LR twin on disk gets one made on the GPU at load time -- Pillow's bicubic resize to
``(w // scale, h // scale)``, byte for byte what sr/Test_dataset.py:24-25 writes (``mulut_amd.resample``).  ``DeviceCropProvider`` has the
kernel write it from the pair's HR slot of the pool straight into its LR slot; ``CropProvider`` copies it back to the host.

``--valEngine`` also scores the tables on the path users deploy: at every validation point, and once after the last iteration, the
current parameters are installed into one ``MuLUTEngine`` (``MuLUT.install_into``: quantised as they will be exported) and every validation image runs through ``engine.pipeline``, scored by ``mulut_eval_y`` and logged with the
test script's line behind the iteration.  ``valid_steps`` rounds after every pass (the module's forward); the deployed cascade does not,
which is 30.605 against 30.608 dB on Set5 for the shipped tables (both print as 30.61) -- with the flag the deployed number is in the log while the run goes on.

``--valResident`` (recommended whenever the run validates) takes the host out of a validation point.  ``DeviceValSet`` decodes the sets
once per run with ``valid_steps``' checks and conversions and keeps them on the device; ``resident_valid_steps`` runs the module per image
and ``mulut_ft_val_pack`` writes its bytes straight into an output pool, ``mulut_eval_plan_run`` scores a whole dataset in one
stream-ordered call, the sums of all datasets are read back once, and the PNGs are copied out on a side stream and encoded by
``--valWorkers`` threads (``ValWriter``) behind the loop.  ``--valSave every|last|never`` picks the points whose files are written.
``resident_engine_valid_steps`` does the same for ``--valEngine``.  The log lines, ``opt.valResults`` and the files are those of the host
loops, bit for bit; a set above a quarter of the free device memory falls back to ``valid_steps`` with one log line.
"""
import argparse
import ctypes
import math
import os
import random
import time

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from .finetune import Adam, MuLUT, MuLUTInterval, MuLUTWide


class _PendingLR:
    """An LR image that DeviceCropProvider will have the resample kernel write straight into its pool slot: only its shape."""
    dtype = np.dtype(np.uint8)

    def __init__(self, shape):
        self.shape, self.size = tuple(shape), int(np.prod(shape))


class CropProvider:
    """Random (LR crop, HR crop) batches, one colour channel each, flips + rot90 as sr/data.py:96-124."""

    def __init__(self, path, scale, patch, batch, seed=None, make_lr=False, log=print, _defer=False):
        self.scale, self.sz, self.batch = scale, patch, batch
        self.rng = random.Random(seed)
        hr_dir = os.path.join(path, "HR")
        self.pairs = []
        for fn in sorted(os.listdir(hr_dir)):
            stem = fn[:-4]
            for lr in (os.path.join(path, "LR", "X%d" % scale, "%sx%d.png" % (stem, scale)),
                       os.path.join(path, "LR_bicubic", "X%d" % scale, fn)):
                if os.path.exists(lr):
                    hr_im = np.array(Image.open(os.path.join(hr_dir, fn)))
                    lr_im = np.array(Image.open(lr))
                    if hr_im.ndim == 2:
                        hr_im, lr_im = hr_im[:, :, None], lr_im[:, :, None]
                    if min(lr_im.shape[:2]) >= patch:
                        self.pairs.append((lr_im, hr_im))
                    break
            else:
                if make_lr:      # no LR twin on disk: the (w // s, h // s) bicubic image of sr/Test_dataset.py:24-25, no modcrop
                    self._make_pair(Image.open(os.path.join(hr_dir, fn)), fn, patch, log, _defer)
        if not self.pairs:
            raise FileNotFoundError("no HR/LR training pairs with LR >= %d px under %s" % (patch, path))

    def _make_pair(self, img, fn, patch, log, defer):
        from .resample import bicubic, resize_image
        s = self.scale
        h, w = img.height // s, img.width // s
        if min(h, w) < max(patch, 1):
            return
        hr_im = np.array(img)
        if img.mode in ("L", "RGB"):
            if hr_im.ndim == 2:
                hr_im = hr_im[:, :, None]
            lr_im = _PendingLR((h, w, hr_im.shape[2])) if defer else bicubic(hr_im, (h, w))
        else:                                  # Pillow on the host, one log line
            lr_im = np.array(resize_image(img, (w, h), log, fn))
            if hr_im.ndim == 2:
                hr_im, lr_im = hr_im[:, :, None], lr_im[:, :, None]
        self.pairs.append((lr_im, hr_im))

    def materialise(self):
        """Make the LR images a deferring scan left pending (on the device, copied back)."""
        from .resample import bicubic
        self.pairs = [(bicubic(hr_im, lr_im.shape[:2]) if isinstance(lr_im, _PendingLR) else lr_im, hr_im) for lr_im, hr_im in self.pairs]

    def next(self):
        ims, lbs = [], []
        for _ in range(self.batch):
            im, lb = self.rng.choice(self.pairs)
            i = self.rng.randint(0, im.shape[0] - self.sz)
            j = self.rng.randint(0, im.shape[1] - self.sz)
            c = self.rng.randrange(im.shape[2])
            s = self.scale
            lb = lb[i * s:(i + self.sz) * s, j * s:(j + self.sz) * s, c]
            im = im[i:i + self.sz, j:j + self.sz, c]
            if self.rng.uniform(0, 1) < 0.5:
                lb, im = np.fliplr(lb), np.fliplr(im)
            if self.rng.uniform(0, 1) < 0.5:
                lb, im = np.flipud(lb), np.flipud(im)
            k = self.rng.choice([0, 1, 2, 3])
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
    """CropProvider's batches, bit for bit for the same seed, cut on the device (mulut_ft_crop_batch): the pairs CropProvider accepts,
    in its order, lie in one uint8 device tensor as the PNGs decode; next() draws pair, i, j, c, the two flips and k per sample from
    random.Random(seed) in CropProvider's order, sends those B x 6 integers through a ring of pinned buffers and launches once on
    the current stream.  next() never waits for the device unless the host is RING batches ahead of it: a slot's event, recorded
    behind its copy, is waited for before the slot is rewritten."""
    RING = 32

    def __init__(self, path, scale, patch, batch, seed=None, max_bytes=None, make_lr=False, log=print):
        host = CropProvider(path, scale, patch, batch, seed, make_lr, log, _defer=True)      # the same scan: the same pairs in the same order
        self.scale, self.sz, self.batch = scale, patch, batch
        self.rng = host.rng
        table, off = np.zeros((len(host.pairs), 10), np.int32), 0
        t64 = table.view(np.int64)                                 # mulut_ft_pair: two 64-bit offsets, then lr_h, lr_w, hr_h, hr_w, ch, pad
        for n, (lr_im, hr_im) in enumerate(host.pairs):
            if lr_im.dtype != np.uint8 or hr_im.dtype != np.uint8 or lr_im.shape[2] != hr_im.shape[2]:
                raise ValueError("pair %d is not a pair of 8-bit images with the same channels (--hostData takes it)" % n)
            t64[n, 0], t64[n, 1] = off, off + lr_im.size
            table[n, 4:9] = lr_im.shape[0], lr_im.shape[1], hr_im.shape[0], hr_im.shape[1], lr_im.shape[2]
            off += lr_im.size + hr_im.size
        self.pool_bytes = off
        if max_bytes is not None and off > max_bytes:
            host.materialise()
            raise TrainingSetTooLarge(off, max_bytes, host)
        self.shapes = [im.shape for im, _ in host.pairs]           # (lr_h, lr_w, ch) per pair: all the draws need
        self.device = torch.empty(0).cuda().device
        self.pool = torch.empty(off, dtype=torch.uint8, device=self.device)
        for n, (lr_im, hr_im) in enumerate(host.pairs):            # image by image: no second copy of the set on the host
            a = int(t64[n, 0])
            hr_slot = self.pool[a + lr_im.size:a + lr_im.size + hr_im.size]
            hr_slot.copy_(torch.from_numpy(np.ascontiguousarray(hr_im).reshape(-1)))
            if isinstance(lr_im, _PendingLR):                      # --makeLR: the kernel writes the pair's LR slot from its HR slot
                from .resample import bicubic
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
        rng, sz, shapes, pairs, ks, rows = self.rng, self.sz, self.shapes, range(len(self.shapes)), [0, 1, 2, 3], []
        for _ in range(self.batch):
            n = rng.choice(pairs)
            h, w, ch = shapes[n]
            i = rng.randint(0, h - sz)
            j = rng.randint(0, w - sz)
            c = rng.randrange(ch)
            lr = rng.uniform(0, 1) < 0.5
            ud = rng.uniform(0, 1) < 0.5
            rows.append((n, i, j, c, lr + 2 * ud, rng.choice(ks)))
        out[:] = rows
        return out

    def next(self):
        if self._ring is None:
            from . import _native
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
        rc = self._lib.mulut_ft_crop_batch(self.device.index, self.pool.data_ptr(), self.pool_bytes, self.table.data_ptr(), len(self.shapes),
                                           draws.data_ptr(), self.batch, self.sz, self.scale, im.data_ptr(), lb.data_ptr(),
                                           self.bad.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
        if rc:
            raise RuntimeError(self._lib.mulut_strerror(rc).decode())
        return im, lb


def valid_steps(net, opt, it, log=print):
    """Twin of sr/3_finetune_lut.py:23-65: datasets under {valDir}/{dataset}/HR with LR_bicubic/X{scale}; a dataset that is
    not on disk is skipped (the reference's Provider would have failed at start-up instead)."""
    from . import _native
    from .metrics import modcrop
    lib = _native.load()
    datasets = _val_datasets(opt)
    was_training = net.training
    net.eval()
    results, per_image = {}, {}
    with torch.no_grad():
        for ds in datasets:
            hr_dir = os.path.join(opt.valDir, ds, "HR")
            if not os.path.isdir(hr_dir):
                continue
            out_dir = os.path.join(opt.valoutDir, ds)
            os.makedirs(out_dir, exist_ok=True)
            psnrs, ssims = [], []
            for fn in sorted(os.listdir(hr_dir)):
                lb = np.array(Image.open(os.path.join(hr_dir, fn)))
                im = np.array(Image.open(os.path.join(opt.valDir, ds, "LR_bicubic", "X%d" % opt.scale, fn)))
                lb = modcrop(lb, opt.scale)                        # sr/data.py:144: rows and columns beyond a multiple of the scale are dropped
                if lb.ndim == 2:                                   # a grey HR and a grey LR are replicated to three channels, each on
                    lb = np.stack([lb] * 3, 2)                     # its own (sr/data.py:145-158)
                if im.ndim == 2:
                    im = np.stack([im] * 3, 2)
                if (im.shape[0] * opt.scale, im.shape[1] * opt.scale) != lb.shape[:2] or im.shape[2] != 3 or lb.shape[2] != 3:      # :163-166
                    raise ValueError("{}/{}: LR {} x scale {} is not the modcropped HR {}".format(ds, fn, im.shape, opt.scale, lb.shape))
                x = torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[None]).astype(np.float32) / 255.0).cuda()
                pred = net(x) * 255.0
                pred_u8 = torch.round(torch.clamp(pred[0].permute(1, 2, 0), 0, 255)).to(torch.uint8).contiguous()
                H, W = pred_u8.shape[:2]
                gt = torch.from_numpy(np.ascontiguousarray(lb)).cuda()
                n = int(lib.mulut_eval_ws_doubles(H, W))
                ws = torch.empty(n, dtype=torch.float64, device="cuda")
                ps, ss = ctypes.c_double(), ctypes.c_double()
                rc = lib.mulut_eval_y(pred_u8.device.index, gt.data_ptr(), pred_u8.data_ptr(), H, W, int(opt.scale), ws.data_ptr(), n,
                                      ctypes.byref(ps), ctypes.byref(ss),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                if rc:
                    raise RuntimeError(lib.mulut_strerror(rc).decode())
                psnrs.append(ps.value)
                ssims.append(ss.value)
                # the reference names the file after the LAST '_'-separated token of "{dataset}_{stem}" (sr/3_finetune_lut.py:41,61):
                # Urban100's img_001.png becomes 001_lutft.png -- kept, a drop-in writes the same names
                Image.fromarray(pred_u8.cpu().numpy()).save(os.path.join(out_dir, '{}_lutft.png'.format((ds + '_' + fn[:-4]).split('_')[-1])))
            if psnrs:
                results[ds] = (float(np.mean(psnrs)), float(np.mean(ssims)))
                per_image[ds] = np.stack([psnrs, ssims], 1)
                log('Iter {} | Dataset {} | AVG PSNR: {:02f}, AVG: SSIM: {:04f}'.format(it, ds, results[ds][0], results[ds][1]))
    net.train(was_training)
    opt.valResults = per_image      # {dataset: float64 array [images, 2]} of this validation, as opt.valEngineResults for the engine's
    return results


def _val_datasets(opt):
    return ['Set5', 'Set14'] if opt.debug else ['Set5', 'Set14', 'B100', 'Urban100', 'Manga109']


def engine_valid_steps(net, engine, opt, it, log=print):
    """The validation sets on the deployed path: the module's current parameters installed into `engine` (install_into), then sr/4_test_lut.py's loop per dataset (:257-317: LR through the cascade, ground truth
    modcropped, grey replicated, Y-PSNR / SSIM) with the test script's summary line behind the iteration.  Returns
    {dataset: float64 array [images, 2]} -- what ``mulut_amd.test_lut`` with device metrics returns for the tables exported now."""
    from .metrics import modcrop
    net.install_into(engine)
    results = {}
    for ds in _val_datasets(opt):
        hr_dir = os.path.join(opt.valDir, ds, "HR")
        if not os.path.isdir(hr_dir):
            continue
        scores = []
        for fn in sorted(os.listdir(hr_dir)):
            im = np.array(Image.open(os.path.join(opt.valDir, ds, "LR_bicubic", "X%d" % opt.scale, fn)))
            gt = modcrop(np.array(Image.open(os.path.join(hr_dir, fn))), opt.scale)
            if im.ndim == 2:
                im = np.stack([im] * 3, axis=2)
            if gt.ndim == 2:
                gt = np.stack([gt] * 3, axis=2)
            out = engine.pipeline(torch.from_numpy(np.ascontiguousarray(im)).to(engine.device))
            scores.append(engine.eval_y(torch.from_numpy(np.ascontiguousarray(gt)).to(engine.device), out, opt.scale))
        if scores:
            results[ds] = np.asarray(scores)
            log('Iter {} | Dataset {} | AVG LUT PSNR: {:.2f} SSIM: {:.4f}'.format(it, ds, np.mean(results[ds][:, 0]), np.mean(results[ds][:, 1])))
    return results


def val_png_name(ds, fn):
    """The reference names a result after the LAST '_'-separated token of "{dataset}_{stem}" (sr/3_finetune_lut.py:41,61)."""
    return '{}_lutft.png'.format((ds + '_' + fn[:-4]).split('_')[-1])


class ValidationSetTooLarge(Exception):
    """The resident validation set needs more device memory than the caller allows."""

    def __init__(self, nbytes, limit):
        super().__init__("validation set of %d bytes exceeds the %d allowed on the device" % (nbytes, limit))
        self.nbytes, self.limit = nbytes, limit


class ValWriter:
    """The PNGs of a validation point, encoded behind the loop by a pool of `workers` threads (Pillow and zlib release the GIL).
    submit() hands over one point's (path, array) list and returns without waiting for its files; it first joins the point before,
    so the files of point k are complete before any file of point k + 1 is begun and at most one point is ever pending.  `ready`,
    if given, is called once on a worker before the point's first file (the wait for the copy that fills the arrays).  A failed
    write is raised by the next join() -- that of the next submit(), or the caller's last one -- not lost."""

    def __init__(self, workers=4, encode=None):
        from concurrent.futures import ThreadPoolExecutor
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix="valpng")
        self._encode = encode or (lambda path, arr: Image.fromarray(arr).save(path))
        self._pending = []

    def submit(self, jobs, ready=None):
        self.join()
        gate = self._pool.submit(ready) if ready is not None else None

        def one(path, arr):
            if gate is not None:
                gate.result()
            self._encode(path, arr)
        self._pending = ([gate] if gate is not None else []) + [self._pool.submit(one, path, arr) for path, arr in jobs]

    def join(self):
        pending, self._pending, first = self._pending, [], None
        for f in pending:                      # every file is waited for, then the first failure is raised
            try:
                f.result()
            except BaseException as e:         # noqa: B902
                first = first or e
        if first is not None:
            raise first

    def close(self):
        try:
            self.join()
        finally:
            self._pool.shutdown(wait=True)


class DeviceValSet:
    """The validation sets of valid_steps / engine_valid_steps, resident on the device for the whole run: built once from
    {valDir}/{dataset}/HR and LR_bicubic/X{scale} with the checks and conversions valid_steps applies per image (modcrop, grey
    replicated to three channels, the shape test and its error text).
      gt_pool   uint8   every ground truth, HWC, back to back
      out_pool  uint8   the same layout: image n's result goes where its ground truth lies in gt_pool
      lr_pool   uint8   every LR image, HWC (what the engine takes)
      lr_f32    float32 the same images as the module takes them, planar [1][3][h][w], the HOST's astype(float32) / 255.0 uploaded
                        once (the device's division is a product with a rounded reciprocal: not the same float for every byte)
      plans     one mulut_eval_plan per dataset over (gt_pool, out_pool); sums: device float64 [images][2], read back once per point
    `max_bytes`: a set that needs more raises ValidationSetTooLarge before anything is allocated on the device."""

    def __init__(self, opt, max_bytes=None, workers=4, encode=None):
        from . import _native
        from .metrics import modcrop
        self.lib = _native.load()
        self.scale = int(opt.scale)
        self.sets, images, gt_bytes, lr_bytes = [], [], 0, 0
        for ds in _val_datasets(opt):
            hr_dir = os.path.join(opt.valDir, ds, "HR")
            if not os.path.isdir(hr_dir):
                continue
            first, files = len(images), sorted(os.listdir(hr_dir))
            for fn in files:
                lb = np.array(Image.open(os.path.join(hr_dir, fn)))
                im = np.array(Image.open(os.path.join(opt.valDir, ds, "LR_bicubic", "X%d" % opt.scale, fn)))
                lb = modcrop(lb, opt.scale)
                if lb.ndim == 2:
                    lb = np.stack([lb] * 3, 2)
                if im.ndim == 2:
                    im = np.stack([im] * 3, 2)
                if (im.shape[0] * opt.scale, im.shape[1] * opt.scale) != lb.shape[:2] or im.shape[2] != 3 or lb.shape[2] != 3:
                    raise ValueError("{}/{}: LR {} x scale {} is not the modcropped HR {}".format(ds, fn, im.shape, opt.scale, lb.shape))
                if lb.dtype != np.uint8 or im.dtype != np.uint8:
                    raise ValueError("{}/{}: not a pair of 8-bit images".format(ds, fn))
                images.append((np.ascontiguousarray(im), np.ascontiguousarray(lb), gt_bytes, lr_bytes))
                gt_bytes, lr_bytes = gt_bytes + lb.size, lr_bytes + im.size
            if files:
                self.sets.append({"name": ds, "files": files, "first": first, "n": len(files), "out_dir": os.path.join(opt.valoutDir, ds)})
        self.gt_bytes, self.lr_bytes = gt_bytes, lr_bytes
        self.nbytes = 2 * gt_bytes + 5 * lr_bytes          # gt + out, LR bytes + LR floats
        if max_bytes is not None and self.nbytes > max_bytes:
            raise ValidationSetTooLarge(self.nbytes, max_bytes)
        self.device = torch.empty(0).cuda().device
        dev = self.device
        self.gt_pool = torch.empty(gt_bytes, dtype=torch.uint8, device=dev)
        self.out_pool = torch.zeros(gt_bytes, dtype=torch.uint8, device=dev)
        self.lr_pool = torch.empty(lr_bytes, dtype=torch.uint8, device=dev)
        self.lr_f32 = torch.empty(lr_bytes, dtype=torch.float32, device=dev)
        self.shapes = []                                   # per image: (gt_off, H, W, lr_off, h, w)
        for im, lb, g, l in images:                        # image by image
            self.gt_pool[g:g + lb.size].copy_(torch.from_numpy(lb.reshape(-1)))
            self.lr_pool[l:l + im.size].copy_(torch.from_numpy(im.reshape(-1)))
            self.lr_f32[l:l + im.size].copy_(torch.from_numpy((np.ascontiguousarray(im.transpose(2, 0, 1)).astype(np.float32) / 255.0).reshape(-1)))
            self.shapes.append((g, lb.shape[0], lb.shape[1], l, im.shape[0], im.shape[1]))
        del images
        self.sums = torch.zeros((len(self.shapes), 2), dtype=torch.float64, device=dev)
        self.sums_host = torch.zeros((len(self.shapes), 2), dtype=torch.float64).pin_memory()
        for s in self.sets:
            items = np.zeros((s["n"], 5), np.int64)        # mulut_eval_item: gt_off, out_off, (H, W) as two int32, the two pool sizes
            for k, (g, H, W, _, _, _) in enumerate(self.shapes[s["first"]:s["first"] + s["n"]]):
                items[k, 0], items[k, 1], items[k, 3], items[k, 4] = g, g, gt_bytes, gt_bytes
                items[k, 2:3].view(np.int32)[:] = (H, W)
            plan = ctypes.c_void_p()
            rc = self.lib.mulut_eval_plan_create(dev.index, items.ctypes.data, s["n"], self.scale, ctypes.byref(plan))
            if rc:
                self.close()
                raise RuntimeError(self.lib.mulut_strerror(rc).decode())
            s["plan"] = plan
        torch.cuda.synchronize(dev)                        # the set is in place whatever stream a validation runs on
        self.writer = ValWriter(workers, encode)
        self.copy_stream, self.copied, self.out_host = None, None, None

    def lr_tensor(self, n):
        _, _, _, l, h, w = self.shapes[n]
        return self.lr_f32[l:l + 3 * h * w].view(1, 3, h, w)

    def lr_bytes_hwc(self, n):
        _, _, _, l, h, w = self.shapes[n]
        return self.lr_pool[l:l + 3 * h * w].view(h, w, 3)

    def out_slot(self, n):
        g, H, W = self.shapes[n][:3]
        return self.out_pool[g:g + 3 * H * W]

    def before_write(self):
        """The output pool is not rewritten before its copy to the host has finished: the current stream waits for that copy (the
        host does not)."""
        if self.copied is not None:
            torch.cuda.current_stream(self.device).wait_event(self.copied)

    def score(self):
        """One mulut_eval_plan_run per dataset on the current stream, then the point's only wait: the sums of all datasets read back
        once.  Returns {dataset: float64 array [images, 2]} of (PSNR, SSIM), mulut_eval_finish applied per image."""
        stream = torch.cuda.current_stream(self.device)
        for s in self.sets:
            rc = self.lib.mulut_eval_plan_run(s["plan"], self.gt_pool.data_ptr(), self.out_pool.data_ptr(),
                                              self.sums[s["first"]:].data_ptr(), ctypes.c_void_p(stream.cuda_stream))
            if rc:
                raise RuntimeError(self.lib.mulut_strerror(rc).decode())
        self.sums_host.copy_(self.sums, non_blocking=True)
        stream.synchronize()
        sums, out = self.sums_host.numpy(), {}
        ps, ss = ctypes.c_double(), ctypes.c_double()
        for s in self.sets:
            rows = []
            for n in range(s["first"], s["first"] + s["n"]):
                _, H, W = self.shapes[n][:3]
                rc = self.lib.mulut_eval_finish(float(sums[n, 0]), float(sums[n, 1]), H, W, self.scale, ctypes.byref(ps), ctypes.byref(ss))
                if rc:
                    raise RuntimeError(self.lib.mulut_strerror(rc).decode())
                rows.append((ps.value, ss.value))
            out[s["name"]] = np.asarray(rows, dtype=np.float64)
        return out

    def save(self):
        """The output pool as it is on the current stream now, to {valoutDir}/{dataset}/ behind the loop: a copy to pinned host memory
        on a side stream, then the writer's threads.  Joins the files of the point before (ValWriter.submit); does not wait for
        its own."""
        self.writer.join()                                 # (the pinned buffer is theirs until they are done)
        if self.out_host is None:
            self.out_host = torch.empty(self.gt_bytes, dtype=torch.uint8).pin_memory()
            self.copy_stream = torch.cuda.Stream(self.device)
        produced = torch.cuda.Event()
        produced.record(torch.cuda.current_stream(self.device))
        self.copy_stream.wait_event(produced)
        with torch.cuda.stream(self.copy_stream):
            self.out_host.copy_(self.out_pool, non_blocking=True)
        copied = torch.cuda.Event()
        copied.record(self.copy_stream)
        self.copied = copied
        host, jobs = self.out_host.numpy(), []
        for s in self.sets:
            os.makedirs(s["out_dir"], exist_ok=True)
            for k, fn in enumerate(s["files"]):
                g, H, W = self.shapes[s["first"] + k][:3]
                jobs.append((os.path.join(s["out_dir"], val_png_name(s["name"], fn)), host[g:g + 3 * H * W].reshape(H, W, 3)))
        self.writer.submit(jobs, ready=copied.synchronize)

    def join(self):
        """Every file submitted so far is on disk (or its failure is raised here)."""
        self.writer.join()

    def close(self):
        for s in self.sets:
            if s.get("plan") is not None:
                self.lib.mulut_eval_plan_destroy(s.pop("plan"))
        if getattr(self, "writer", None) is not None:
            self.writer.close()


def _val_saves(opt, it):
    """--valSave: every point's files, the final validation point's only, or none."""
    mode = getattr(opt, "valSave", "every")
    if mode == "last":
        step = getattr(opt, "valStep", 0)
        return it == (((opt.totalIter // step) * step or 1) if step else 1)      # (iteration 1 is the only point of a run shorter than valStep)
    return mode == "every"


def resident_valid_steps(net, vset, opt, it, log=print):
    """valid_steps from a DeviceValSet: per image the module under no_grad and one mulut_ft_val_pack straight into the image's slot of
    the output pool, per dataset one mulut_eval_plan_run, one read-back at the end of the point, the PNGs behind the loop.  The same
    log lines, return value and opt.valResults as valid_steps, the same doubles."""
    lib, was_training = vset.lib, net.training
    net.eval()
    vset.before_write()
    stream = ctypes.c_void_p(torch.cuda.current_stream(vset.device).cuda_stream)
    with torch.no_grad():
        for n in range(len(vset.shapes)):
            pred = net(vset.lr_tensor(n)).contiguous()
            _, H, W = vset.shapes[n][:3]
            if tuple(pred.shape) != (1, 3, H, W) or pred.dtype != torch.float32:
                raise ValueError("the module's output {} is not the ground truth's [1, 3, {}, {}]".format(tuple(pred.shape), H, W))
            rc = lib.mulut_ft_val_pack(vset.device.index, pred.data_ptr(), H, W, vset.out_slot(n).data_ptr(), stream)
            if rc:
                raise RuntimeError(lib.mulut_strerror(rc).decode())
    per_image = vset.score()
    if _val_saves(opt, it):
        vset.save()
    results = {}
    for ds, rows in per_image.items():
        results[ds] = (float(np.mean(rows[:, 0].tolist())), float(np.mean(rows[:, 1].tolist())))
        log('Iter {} | Dataset {} | AVG PSNR: {:02f}, AVG: SSIM: {:04f}'.format(it, ds, results[ds][0], results[ds][1]))
    net.train(was_training)
    opt.valResults = per_image
    return results


def resident_engine_valid_steps(net, engine, vset, opt, it, log=print):
    """engine_valid_steps from a DeviceValSet: install_into, engine.pipeline from the uint8 LR pool into the output pool, the same
    plans and read-back as resident_valid_steps.  The lines and arrays of engine_valid_steps.  (It saves no files, as that does not.)"""
    net.install_into(engine)
    vset.before_write()
    for n in range(len(vset.shapes)):
        engine.pipeline(vset.lr_bytes_hwc(n), out=vset.out_slot(n))
    results = vset.score()
    for ds in results:
        log('Iter {} | Dataset {} | AVG LUT PSNR: {:.2f} SSIM: {:.4f}'.format(it, ds, np.mean(results[ds][:, 0]), np.mean(results[ds][:, 1])))
    return results


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    # the flags sr/3_finetune_lut.py reads from TrainOptions (common/option.py:15-29,160-187)
    p.add_argument('--scale', '-r', type=int, default=4)
    p.add_argument('--stages', type=int, default=2)
    p.add_argument('--modes', type=str, default='sdy')
    p.add_argument('--interval', type=int, default=4)
    p.add_argument('--expDir', '-e', type=str, required=True)
    p.add_argument('--batchSize', type=int, default=32)
    p.add_argument('--cropSize', type=int, default=48)
    p.add_argument('--trainDir', type=str, default="../data/DIV2K")
    p.add_argument('--valDir', type=str, default='../data/SRBenchmark')
    p.add_argument('--valStep', type=int, default=2000, help='validate every N iterations (and at iteration 1); 0 = never')
    p.add_argument('--valoutDir', type=str, default=None, help='default: {expDir}/val')
    p.add_argument('--debug', default=False, action='store_true')
    p.add_argument('--totalIter', type=int, default=200000)
    p.add_argument('--displayStep', type=int, default=100)
    p.add_argument('--lr0', type=float, default=1e-3)
    p.add_argument('--lr1', type=float, default=1e-4)
    p.add_argument('--weightDecay', type=float, default=0)
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--hostData', default=False, action='store_true',
                   help='cut the batches on the host (CropProvider, the reference\'s path) instead of on the device')
    p.add_argument('--makeLR', default=False, action='store_true',
                   help='an HR image without an LR twin on disk gets one made on the GPU at load time: Pillow\'s bicubic resize to '
                        '(w // scale, h // scale), the bytes sr/Test_dataset.py writes')
    p.add_argument('--valEngine', default=False, action='store_true',
                   help='also score the current tables on the inference engine (the deployed path) at every validation point and '
                        'after the last iteration')
    p.add_argument('--valResident', default=False, action='store_true',
                   help='validate from a device-resident set (DeviceValSet): decoded and uploaded once per run, scored in one call per '
                        'dataset, PNGs written behind the loop -- the same log lines, numbers and files as without it')
    p.add_argument('--valSave', choices=['every', 'last', 'never'], default='every',
                   help='with --valResident: write the PNGs of every validation point, of the final one only, or none')
    p.add_argument('--valWorkers', type=int, default=4, help='with --valResident: threads that encode the PNGs behind the loop')
    p.add_argument('--valMaxBytes', type=int, default=None,
                   help='with --valResident: device bytes the resident set may take (default: a quarter of the free device memory); '
                        'a larger set is validated by the host loop')
    return p


class FinetuneRun:
    """One fine-tune run (sr/3_finetune_lut.py:80-171) in three parts: what is built before the loop, one iteration, and what follows
    the last one.  ``finetune()`` is ``run = FinetuneRun(opt, log); step() x totalIter; run.finish()``; a caller that drives the steps
    itself can look at ``net``, ``optim``, ``sched`` and ``loss_buf`` between two of them."""

    def __init__(self, opt, log=print):
        self.opt, self.log = opt, log
        wide = any(m in "eho" for m in opt.modes)      # the reference's module stops at s, d, y (sr/model.py:119-121)
        self.net = (MuLUTWide if wide else MuLUTInterval if opt.interval in (5, 6) else MuLUT)(opt.expDir, opt.stages, list(opt.modes), upscale=opt.scale, interval=opt.interval).cuda()
        params = [p for p in self.net.parameters() if p.requires_grad]
        # the reference's Adam as one launch over the six tables, its arithmetic in float64 (torch's default is ~10 launches per step; its
        # fused=True is one, but strays from float64 Adam by hundreds of float32 ulps on an element that lands near zero, as every float32 Adam does)
        self.optim = Adam(params, lr=opt.lr0, betas=(0.9, 0.999), eps=1e-8, weight_decay=opt.weightDecay)
        if opt.lr1 < 0:                                                        # sr/3_finetune_lut.py:89-95
            lf = lambda x: (((1 + math.cos(x * math.pi / opt.totalIter)) / 2) ** 1.0) * 0.8 + 0.2   # noqa: E731
        else:
            lr_b = opt.lr1 / opt.lr0
            lr_a = 1 - lr_b
            lf = lambda x: (((1 + math.cos(x * math.pi / opt.totalIter)) / 2) ** 1.0) * lr_a + lr_b   # noqa: E731
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.optim, lr_lambda=lf)
        make_lr = getattr(opt, "makeLR", False)
        if getattr(opt, "hostData", False):
            self.data = CropProvider(opt.trainDir, opt.scale, opt.cropSize, opt.batchSize, opt.seed, make_lr, log)
        else:
            try:      # the set stays on the device for the whole run: at most half of what is free now
                self.data = DeviceCropProvider(opt.trainDir, opt.scale, opt.cropSize, opt.batchSize, opt.seed, max_bytes=torch.cuda.mem_get_info()[0] // 2,
                                               make_lr=make_lr, log=log)
            except TrainingSetTooLarge as e:
                log("{} | training set of {} bytes exceeds half the free device memory ({}): batches are cut on the host".format(opt.expDir, e.nbytes, e.limit))
                self.data = e.host
        if getattr(opt, "valoutDir", None) is None:
            opt.valoutDir = os.path.join(opt.expDir, "val")
        self.engine, self.engine_at = None, 0
        if getattr(opt, "valEngine", False):      # one engine for the run: later installs rewrite its tables in place
            from .engine import MuLUTEngine
            self.engine = MuLUTEngine(next(self.net.parameters()).device.index).configure(opt.stages, opt.modes, opt.scale, opt.interval)
            opt.valEngineResults = {}              # {dataset: [images, 2]} of the last engine validation, for callers
        self.vset = None
        if getattr(opt, "valResident", False) and os.path.isdir(getattr(opt, "valDir", "")) and (getattr(opt, "valStep", 0) or self.engine is not None):
            limit = getattr(opt, "valMaxBytes", None)
            try:      # resident for the whole run: at most a quarter of what is free now
                self.vset = DeviceValSet(opt, max_bytes=torch.cuda.mem_get_info()[0] // 4 if limit is None else limit, workers=getattr(opt, "valWorkers", 4))
            except ValidationSetTooLarge as e:
                log("{} | validation set of {} bytes exceeds the {} allowed on the device: validation runs on the host loop".format(opt.expDir, e.nbytes, e.limit))
        # the loop never waits for the device per step: every loss goes into this vector, read at the display points and at the end
        self.loss_buf = torch.zeros(opt.totalIter, dtype=torch.float32, device="cuda")
        self.losses, self.t_mark, self.i = [], time.time(), 0

    def step(self):
        """Iteration self.i + 1 (sr/3_finetune_lut.py:118-159).  Returns nothing: no wait for the device but at a display point."""
        opt, log, net = self.opt, self.log, self.net
        self.i += 1
        i, losses = self.i, self.losses
        im, lb = self.data.next()
        self.optim.zero_grad()
        loss = F.mse_loss(net(im), lb)
        loss.backward()
        self.optim.step()
        self.sched.step()
        self.loss_buf[i - 1] = loss.detach()
        if i % opt.displayStep == 0:
            losses.extend(self.loss_buf[len(losses):i].tolist())        # (waits for the device)
            # rT: wall time per iteration since the last display point (or the start), validation left out
            log("{} | Iter:{:6d}, Sample:{:6d}, GPixel:{:.2e}, rT:{:.4f}".format(opt.expDir, i, i * opt.batchSize,
                                                                               sum(losses[i - opt.displayStep:i]) / opt.displayStep,
                                                                               (time.time() - self.t_mark) / opt.displayStep))
            self.t_mark = time.time()
        if getattr(opt, "valStep", 0) and (i % opt.valStep == 0 or i == 1) and os.path.isdir(getattr(opt, "valDir", "")):   # :152-158
            t_val = time.time()
            if self.vset is not None:
                resident_valid_steps(net, self.vset, opt, i, log)
            else:
                valid_steps(net, opt, i, log)
            if self.engine is not None:
                opt.valEngineResults, self.engine_at = self._engine_valid(i), i
            self.t_mark += time.time() - t_val

    def _engine_valid(self, it):
        if self.vset is not None:
            return resident_engine_valid_steps(self.net, self.engine, self.vset, self.opt, it, self.log)
        return engine_valid_steps(self.net, self.engine, self.opt, it, self.log)

    def finish(self):
        """The last read-back, the engine's score of the tables as they are exported, the export (:162-171); with --valResident every
        PNG is on disk when this returns, and a write that failed is raised here.  Returns the losses."""
        opt, log, net, data, losses = self.opt, self.log, self.net, self.data, self.losses
        losses.extend(self.loss_buf[len(losses):self.i].tolist())
        try:
            if self.engine is not None:
                if self.engine_at != opt.totalIter and os.path.isdir(getattr(opt, "valDir", "")):      # the tables as they are exported below
                    opt.valEngineResults = self._engine_valid(opt.totalIter)
                self.engine.close()
        finally:
            if self.vset is not None:
                self.vset.close()
        if isinstance(data, DeviceCropProvider) and int(data.bad.item()):
            raise RuntimeError("mulut_ft_crop_batch refused %d samples" % int(data.bad.item()))
        for key, table in net.export_int8().items():                          # :162-169
            np.save(os.path.join(opt.expDir, "LUT_ft_x{}_{}bit_int8_{}.npy".format(opt.scale, opt.interval, key)), table)
        log("Finetuned LUT saved to {}".format(opt.expDir))
        return losses


def finetune(opt, log=print):
    run = FinetuneRun(opt, log)
    for _ in range(opt.totalIter):
        run.step()
    return run.finish()


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if opt.debug:                                              # common/option.py:147-151
        opt.displayStep, opt.valStep, opt.totalIter = 10, 50, min(opt.totalIter, 200)
    return finetune(opt)


if __name__ == "__main__":
    main()
