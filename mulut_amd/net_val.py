"""Validation of a trained network on the fused forward: the twin of sr/1_train_model.py:70-117 (`valid_steps`) over a NetEngine,
built from what the fine-tune validation already has (ft_val.iter_val_pairs, the naming scheme of ft_val.val_png_name)."""
import os

import numpy as np
import torch
from PIL import Image

from . import ft_val
from .metrics import _O, _T, psnr, rgb2ycbcr


def net_png_name(ds, fn, suffix="net"):
    """ft_val.val_png_name's scheme (the last '_'-separated token of "{dataset}_{stem}", sr/1_train_model.py:109-114) with the
    suffixes of the training script: _net, _input, _gt."""
    return '{}_{}.png'.format((ds + '_' + fn[:-4]).split('_')[-1], suffix)


class NetValSet(ft_val.DeviceValSet):
    """The validation sets of net_valid_steps resident on the device: ft_val.DeviceValSet without the float32 LR pool (the fused
    forward reads bytes), results named by net_png_name, one NetPlan per dataset from lr_pool into out_pool, made for the engine of
    the first validation point and kept, and the host half of a point: one read-back of the output pool, scored there as
    net_valid_steps scores.  No mulut_eval_plan is made (their PSNR is float64 arithmetic, not the host loop's), and DeviceValSet's
    `score`, `save` and `before_write` -- the device score and the side-stream copy of the fine-tune path -- are refused here: a point
    is `plans`, `fetch`, `score_host`, `save_host`."""

    def __init__(self, opt, max_bytes=None, workers=4, encode=None):
        from concurrent.futures import ThreadPoolExecutor
        self._plans, self.inputs_saved, self.first_it = None, False, None      # first_it: the iteration of the run's first point
        self._gt_y, self._scorers = None, ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix="valpsnr")
        super().__init__(opt, max_bytes, workers, encode, lr_float=False, png_name=net_png_name, eval_plans=False)

    def _not_here(self, *a, **kw):
        raise RuntimeError("NetValSet scores and saves from one read-back: fetch(), score_host(), save_host()")

    score = save = before_write = _not_here

    def plans(self, engine):
        if self._plans is None or self._plans[0] is not engine:
            self._close_plans()
            made = []
            self._plans = (engine, made)
            for s in self.sets:
                made.append(engine.plan([(sh.lr_off, sh.gt_off, sh.h, sh.w, self.lr_bytes, self.gt_bytes)
                                         for sh in self.shapes[s["first"]:s["first"] + s["n"]]]))
        return self._plans[1]

    def input_jobs(self):
        """The (path, array) jobs of every image's _input.png and _gt.png: the two pools read back, once in a run."""
        lr, gt, jobs = self.lr_pool.cpu().numpy(), self.gt_pool.cpu().numpy(), []
        for s in self.sets:
            os.makedirs(s["out_dir"], exist_ok=True)
            for k, fn in enumerate(s["files"]):
                sh = self.shapes[s["first"] + k]
                jobs.append((os.path.join(s["out_dir"], net_png_name(s["name"], fn, "input")), lr[sh.lr_off:sh.lr_off + 3 * sh.h * sh.w].reshape(sh.h, sh.w, 3)))
                jobs.append((os.path.join(s["out_dir"], net_png_name(s["name"], fn, "gt")), gt[sh.gt_off:sh.gt_off + 3 * sh.H * sh.W].reshape(sh.H, sh.W, 3)))
        return jobs

    def fetch(self):
        """The output pool as it is on the current stream now, in pinned host memory: the point's one read-back and its one wait.
        Joins the files of the point before first (the buffer is their source)."""
        self.writer.join()
        if self.out_host is None:
            self.out_host = torch.empty(self.gt_bytes, dtype=torch.uint8).pin_memory()
        self.out_host.copy_(self.out_pool, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self.out_host.numpy()

    def _image(self, host, n):
        sh = self.shapes[n]
        return host[sh.gt_off:sh.gt_off + 3 * sh.H * sh.W].reshape(sh.H, sh.W, 3)

    def score_host(self, host):
        """{dataset: float64 [images]} of metrics.psnr -- net_valid_steps' own arithmetic, so its doubles -- between the results in
        `host` (fetch()) and the ground truths, whose float32 luma is made once in a run; an image a call on the set's worker threads
        (NumPy releases the GIL in these loops)."""
        if self._gt_y is None:
            gt = self.gt_pool.cpu().numpy()
            self._gt_y = list(self._scorers.map(lambda n: luma32(self._image(gt, n)), range(len(self.shapes))))
        one = lambda n: psnr(luma32(self._image(host, n)), self._gt_y[n], self.scale)      # noqa: E731
        scores = list(self._scorers.map(one, range(len(self.shapes))))
        return {s["name"]: np.asarray(scores[s["first"]:s["first"] + s["n"]], dtype=np.float64) for s in self.sets}

    def save_host(self, host, extra=()):
        """The results in `host` to {valoutDir}/{dataset}/ behind the loop, `extra` jobs behind them; does not wait for its files."""
        jobs = []
        for s in self.sets:
            os.makedirs(s["out_dir"], exist_ok=True)
            jobs += [(os.path.join(s["out_dir"], self.png_name(s["name"], fn)), self._image(host, s["first"] + k)) for k, fn in enumerate(s["files"])]
        self.writer.submit(jobs + list(extra))

    def _close_plans(self):
        if self._plans is not None:
            for p in self._plans[1]:
                p.close()
            self._plans = None

    def close(self):
        self._close_plans()
        self._scorers.shutdown(wait=True)
        super().close()


def luma32(img):
    """np.array(rgb2ycbcr(img)[:, :, 0], dtype=np.float32), the Y plane as metrics.psnr takes it, without the two chroma columns: the
    same float64 products added in the same order (tests/test_net_list_cpu.py holds the two to equal bits)."""
    flat = np.reshape(img, (-1, 3)).astype(np.float64)
    y = flat[:, 0] * _T[0, 0] + flat[:, 1] * _T[0, 1] + flat[:, 2] * _T[0, 2] + _O[0]
    return y.astype(np.float32).reshape(img.shape[:2])


def resident_net_valid_steps(net_engine, vset, opt, it, log=print):
    """net_valid_steps from a NetValSet: per dataset one NetPlan.run (the list form of the cascade, `stages` launches, HWC bytes of
    lr_pool to HWC bytes of out_pool), then the point's one read-back and one wait -- the output pool to pinned host memory -- the
    PSNRs by metrics.psnr on the set's worker threads, and the PNGs from the same host copy behind the loop.  The same log lines and
    return value as net_valid_steps, the same doubles: the score is that loop's own float32 arithmetic on the same bytes
    (mulut_eval_finish works in float64 behind the mean and prints other digits, so `score()` is not used here).  Files per
    --valSave: `every` writes each point's _net.png, and _input.png / _gt.png once, with the run's first point if its iteration
    is below 10000 (the host loop rewrites them with the same bytes at every such point); `last` writes all three kinds with the
    final point only; `never` none."""
    for plan in vset.plans(net_engine):
        plan.run(vset.lr_pool, vset.out_pool)
    host = vset.fetch()
    results = vset.score_host(host)
    if vset.first_it is None:
        vset.first_it = it
    if ft_val._val_saves(opt, it):
        first, vset.inputs_saved = not vset.inputs_saved, True
        vset.save_host(host, vset.input_jobs() if first and vset.first_it < 10000 else ())
    for ds in results:
        log('Iter {} | Dataset {} | AVG Val PSNR: {}'.format(it, ds, np.mean(results[ds])))
    return results


def net_valid_steps(net_engine, opt, it, log=print):
    """Each validation image through NetEngine.predict (bytes to bytes on the device), Y-PSNR with shave = scale on the host
    (:103-104), `{valoutDir}/{dataset}/{name}_net.png` (and _input / _gt below iteration 10000, :106-111), one line per dataset.
    Returns {dataset: float64 array [images]} of the PSNRs."""
    results = {}
    for ds, pairs in ft_val._by_dataset(opt):
        out_dir = os.path.join(opt.valoutDir, ds)
        os.makedirs(out_dir, exist_ok=True)
        psnrs = []
        for _, fn, im, lb in pairs:
            x = torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[None])).to(net_engine.device)
            pred = net_engine.predict(x)[0].permute(1, 2, 0).contiguous().cpu().numpy()
            psnrs.append(psnr(rgb2ycbcr(pred)[:, :, 0], rgb2ycbcr(lb)[:, :, 0], opt.scale))
            if it < 10000:
                Image.fromarray(im).save(os.path.join(out_dir, net_png_name(ds, fn, "input")))
                Image.fromarray(lb).save(os.path.join(out_dir, net_png_name(ds, fn, "gt")))
            Image.fromarray(pred).save(os.path.join(out_dir, net_png_name(ds, fn)))
        results[ds] = np.asarray(psnrs, dtype=np.float64)
        log('Iter {} | Dataset {} | AVG Val PSNR: {}'.format(it, ds, np.mean(results[ds])))
    return results
