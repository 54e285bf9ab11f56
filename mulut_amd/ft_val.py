"""Validation of the fine-tune driver (mulut_amd/finetune_lut.py): ``iter_val_pairs``, the only loop of the driver that opens a validation
image; the reference's host loop ``valid_steps`` (sr/3_finetune_lut.py:23-65) and its twin on the deployed path, ``engine_valid_steps``;
the same two from a device-resident set (``DeviceValSet``, ``resident_*``) with the PNGs written behind the loop (``ValWriter``)."""
import collections
import ctypes
import itertools
import os

import numpy as np
import torch
from PIL import Image

from . import _native
from .engine import eval_y


def _val_datasets(opt):
    return ['Set5', 'Set14'] if opt.debug else ['Set5', 'Set14', 'B100', 'Urban100', 'Manga109']


def iter_val_pairs(opt):
    """(dataset, file name, lr, gt) of every validation pair as contiguous H x W x 3 arrays: the datasets under {valDir}/{dataset}/HR
    with LR_bicubic/X{scale}, files in sorted order; a dataset that is not on disk is skipped (the reference's Provider would have
    failed at start-up instead).  Lazy: a pair is decoded when it is asked for."""
    from .metrics import modcrop
    for ds in _val_datasets(opt):
        hr_dir = os.path.join(opt.valDir, ds, "HR")
        if not os.path.isdir(hr_dir):
            continue
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
            yield ds, fn, np.ascontiguousarray(im), np.ascontiguousarray(lb)


def _by_dataset(opt):
    """iter_val_pairs, one (dataset, its pairs) at a time."""
    return itertools.groupby(iter_val_pairs(opt), key=lambda pair: pair[0])


def val_png_name(ds, fn):
    """The reference names a result after the LAST '_'-separated token of "{dataset}_{stem}" (sr/3_finetune_lut.py:41,61):
    Urban100's img_001.png becomes 001_lutft.png -- kept, a drop-in writes the same names."""
    return '{}_lutft.png'.format((ds + '_' + fn[:-4]).split('_')[-1])


def valid_steps(net, opt, it, log=print):
    """Twin of sr/3_finetune_lut.py:23-65 over iter_val_pairs: each image through the module, scored on the device (eval_y) and saved."""
    was_training = net.training
    net.eval()
    results, per_image = {}, {}
    with torch.no_grad():
        for ds, pairs in _by_dataset(opt):
            out_dir = os.path.join(opt.valoutDir, ds)
            os.makedirs(out_dir, exist_ok=True)
            scores = []
            for _, fn, im, lb in pairs:
                x = torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[None]).astype(np.float32) / 255.0).cuda()
                pred = net(x) * 255.0
                pred_u8 = torch.round(torch.clamp(pred[0].permute(1, 2, 0), 0, 255)).to(torch.uint8).contiguous()
                scores.append(eval_y(torch.from_numpy(lb).cuda(), pred_u8, opt.scale))
                Image.fromarray(pred_u8.cpu().numpy()).save(os.path.join(out_dir, val_png_name(ds, fn)))
            per_image[ds] = np.asarray(scores)
            results[ds] = (float(np.mean(per_image[ds][:, 0].tolist())), float(np.mean(per_image[ds][:, 1].tolist())))
            log('Iter {} | Dataset {} | AVG PSNR: {:02f}, AVG: SSIM: {:04f}'.format(it, ds, results[ds][0], results[ds][1]))
    net.train(was_training)
    opt.valResults = per_image      # {dataset: float64 array [images, 2]} of this validation, as opt.valEngineResults for the engine's
    return results


def engine_valid_steps(net, engine, opt, it, log=print):
    """The validation sets on the deployed path: the module's current parameters installed into `engine` (install_into), then sr/4_test_lut.py's loop per dataset (:257-317: LR through the cascade, ground truth
    modcropped, grey replicated, Y-PSNR / SSIM) with the test script's summary line behind the iteration.  Returns
    {dataset: float64 array [images, 2]} -- what ``mulut_amd.test_lut`` with device metrics returns for the tables exported now."""
    net.install_into(engine)
    results = {}
    for ds, pairs in _by_dataset(opt):
        scores = []
        for _, _, im, gt in pairs:
            out = engine.pipeline(torch.from_numpy(im).to(engine.device))
            scores.append(engine.eval_y(torch.from_numpy(gt).to(engine.device), out, opt.scale))
        results[ds] = np.asarray(scores)
        log('Iter {} | Dataset {} | AVG LUT PSNR: {:.2f} SSIM: {:.4f}'.format(it, ds, np.mean(results[ds][:, 0]), np.mean(results[ds][:, 1])))
    return results


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


# an image of a DeviceValSet: ground truth and result H x W x 3 at byte gt_off of gt_pool / out_pool, LR h x w x 3 at lr_off of lr_pool / lr_f32
ValShape = collections.namedtuple("ValShape", "gt_off H W lr_off h w")


class DeviceValSet:
    """The validation sets of valid_steps / engine_valid_steps, resident on the device for the whole run: built once from
    iter_val_pairs, so with the checks and conversions valid_steps applies per image (modcrop, grey replicated to three channels,
    the shape test and its error text).
      gt_pool   uint8   every ground truth, HWC, back to back
      out_pool  uint8   the same layout: image n's result goes where its ground truth lies in gt_pool
      lr_pool   uint8   every LR image, HWC (what the engine takes)
      lr_f32    float32 the same images as the module takes them, planar [1][3][h][w], the HOST's astype(float32) / 255.0 uploaded
                        once (the device's division is a product with a rounded reciprocal: not the same float for every byte)
      plans     one mulut_eval_plan per dataset over (gt_pool, out_pool); sums: device float64 [images][2], read back once per point
    `max_bytes`: a set that needs more raises ValidationSetTooLarge before anything is allocated on the device.
    `lr_float` False leaves lr_f32 out (None): the three byte pools are all the network's validation reads (net_val).
    `png_name`: (dataset, file name) -> the name `save` writes the result under; val_png_name if None.
    `eval_plans` False makes no mulut_eval_plan: a set whose owner scores otherwise (net_val.NetValSet); `score` is then not to be called."""

    def __init__(self, opt, max_bytes=None, workers=4, encode=None, lr_float=True, png_name=None, eval_plans=True):
        self.lib = _native.load()
        self.scale = int(opt.scale)
        self.png_name = png_name or val_png_name
        self.sets, images, gt_bytes, lr_bytes = [], [], 0, 0
        for ds, pairs in _by_dataset(opt):
            first, files = len(images), []
            for _, fn, im, lb in pairs:
                if lb.dtype != np.uint8 or im.dtype != np.uint8:
                    raise ValueError("{}/{}: not a pair of 8-bit images".format(ds, fn))
                files.append(fn)
                images.append((im, lb, gt_bytes, lr_bytes))
                gt_bytes, lr_bytes = gt_bytes + lb.size, lr_bytes + im.size
            self.sets.append({"name": ds, "files": files, "first": first, "n": len(files), "out_dir": os.path.join(opt.valoutDir, ds)})
        self.gt_bytes, self.lr_bytes = gt_bytes, lr_bytes
        self.nbytes = self.pool_bytes(gt_bytes, lr_bytes, lr_float)
        if max_bytes is not None and self.nbytes > max_bytes:
            raise ValidationSetTooLarge(self.nbytes, max_bytes)
        dev = self.device = torch.empty(0).cuda().device
        self.gt_pool = torch.empty(gt_bytes, dtype=torch.uint8, device=dev)
        self.out_pool = torch.zeros(gt_bytes, dtype=torch.uint8, device=dev)
        self.lr_pool = torch.empty(lr_bytes, dtype=torch.uint8, device=dev)
        self.lr_f32 = torch.empty(lr_bytes, dtype=torch.float32, device=dev) if lr_float else None
        self.shapes = []                                   # a ValShape per image
        for im, lb, g, l in images:                        # image by image
            self.gt_pool[g:g + lb.size].copy_(torch.from_numpy(lb.reshape(-1)))
            self.lr_pool[l:l + im.size].copy_(torch.from_numpy(im.reshape(-1)))
            if lr_float:
                self.lr_f32[l:l + im.size].copy_(torch.from_numpy((np.ascontiguousarray(im.transpose(2, 0, 1)).astype(np.float32) / 255.0).reshape(-1)))
            self.shapes.append(ValShape(g, lb.shape[0], lb.shape[1], l, im.shape[0], im.shape[1]))
        del images
        self.sums = torch.zeros((len(self.shapes), 2), dtype=torch.float64, device=dev)
        self.sums_host = torch.zeros((len(self.shapes), 2), dtype=torch.float64).pin_memory()
        for s in (self.sets if eval_plans else []):
            items = np.zeros((s["n"], 5), np.int64)        # mulut_eval_item: gt_off, out_off, (H, W) as two int32, the two pool sizes
            for k, sh in enumerate(self.shapes[s["first"]:s["first"] + s["n"]]):
                items[k, 0], items[k, 1], items[k, 3], items[k, 4] = sh.gt_off, sh.gt_off, gt_bytes, gt_bytes
                items[k, 2:3].view(np.int32)[:] = (sh.H, sh.W)
            plan = ctypes.c_void_p()
            rc = self.lib.mulut_eval_plan_create(dev.index, items.ctypes.data, s["n"], self.scale, ctypes.byref(plan))
            if rc:
                self.close()
            _native.check(rc)
            s["plan"] = plan
        torch.cuda.synchronize(dev)                        # the set is in place whatever stream a validation runs on
        self.writer = ValWriter(workers, encode)
        self.copy_stream, self.copied, self.out_host = None, None, None

    @staticmethod
    def pool_bytes(gt_bytes, lr_bytes, lr_float=True):
        """Device bytes of the pools: ground truths and results, the LR bytes, and with `lr_float` the LR floats."""
        return 2 * gt_bytes + (5 if lr_float else 1) * lr_bytes

    def lr_tensor(self, n):
        _, _, _, l, h, w = self.shapes[n]
        return self.lr_f32[l:l + 3 * h * w].view(1, 3, h, w)

    def lr_bytes_hwc(self, n):
        _, _, _, l, h, w = self.shapes[n]
        return self.lr_pool[l:l + 3 * h * w].view(h, w, 3)

    def out_slot(self, n):
        g, H, W, _, _, _ = self.shapes[n]
        return self.out_pool[g:g + 3 * H * W]

    def before_write(self):
        """The output pool is not rewritten before its copy to the host has finished: the current stream waits for that copy (the
        host does not)."""
        if self.copied is not None:
            torch.cuda.current_stream(self.device).wait_event(self.copied)

    def score(self):
        """One mulut_eval_plan_run per dataset on the current stream, then the point's only wait: the sums of all datasets read back
        once.  Returns {dataset: float64 array [images, 2]} of (PSNR, SSIM), mulut_eval_finish applied per image."""
        stream = _native.stream_ptr(self.device)
        for s in self.sets:
            _native.check(self.lib.mulut_eval_plan_run(s["plan"], self.gt_pool.data_ptr(), self.out_pool.data_ptr(),
                                                       self.sums[s["first"]:].data_ptr(), stream))
        self.sums_host.copy_(self.sums, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        sums, out = self.sums_host.numpy(), {}
        ps, ss = ctypes.c_double(), ctypes.c_double()
        for s in self.sets:
            rows = []
            for n in range(s["first"], s["first"] + s["n"]):
                sh = self.shapes[n]
                _native.check(self.lib.mulut_eval_finish(float(sums[n, 0]), float(sums[n, 1]), sh.H, sh.W, self.scale, ctypes.byref(ps), ctypes.byref(ss)))
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
                sh = self.shapes[s["first"] + k]
                jobs.append((os.path.join(s["out_dir"], self.png_name(s["name"], fn)),
                             host[sh.gt_off:sh.gt_off + 3 * sh.H * sh.W].reshape(sh.H, sh.W, 3)))
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
    if opt.valSave == "last":      # (iteration 1 is the only point of a run shorter than valStep)
        return it == (((opt.totalIter // opt.valStep) * opt.valStep or 1) if opt.valStep else 1)
    return opt.valSave == "every"


def resident_valid_steps(net, vset, opt, it, log=print):
    """valid_steps from a DeviceValSet: per image the module under no_grad and one mulut_ft_val_pack straight into the image's slot of
    the output pool, per dataset one mulut_eval_plan_run, one read-back at the end of the point, the PNGs behind the loop.  The same
    log lines, return value and opt.valResults as valid_steps, the same doubles."""
    lib, was_training = vset.lib, net.training
    net.eval()
    vset.before_write()
    stream = _native.stream_ptr(vset.device)
    with torch.no_grad():
        for n, (_, H, W, _, _, _) in enumerate(vset.shapes):
            pred = net(vset.lr_tensor(n)).contiguous()
            if tuple(pred.shape) != (1, 3, H, W) or pred.dtype != torch.float32:
                raise ValueError("the module's output {} is not the ground truth's [1, 3, {}, {}]".format(tuple(pred.shape), H, W))
            _native.check(lib.mulut_ft_val_pack(vset.device.index, pred.data_ptr(), H, W, vset.out_slot(n).data_ptr(), stream))
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
