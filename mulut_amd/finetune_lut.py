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
``--deterministic`` builds the module with ``deterministic=True``: every stage's backward is ``mulut_ft_exact_stage_backward`` (64-bit
fixed-point gradient sums), and with a fixed ``--seed`` two runs write the same ``LUT_ft_*.npy`` bytes.  Everything else in the loop is as
without the flag.
The providers, their scan and their draw are defined in ``mulut_amd.ft_data``, everything named above that validates in
``mulut_amd.ft_val``; this module is the parser and the loop, and carries those names as its own.
"""
import argparse
import math
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from .finetune import Adam, MuLUT, MuLUTInterval, MuLUTWide
from .ft_data import CropProvider, DeviceCropProvider, TrainingSetTooLarge, _PendingLR, draw_sample, scan_pairs  # noqa: F401
from .ft_val import (DeviceValSet, ValidationSetTooLarge, ValShape, ValWriter, _val_datasets, _val_saves, engine_valid_steps,  # noqa: F401
                     iter_val_pairs, resident_engine_valid_steps, resident_valid_steps, val_png_name, valid_steps)


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
    p.add_argument('--deterministic', default=False, action='store_true',
                   help='bit-reproducible training: the backward kernels sum every gradient in 64-bit fixed point instead of with '
                        'float32 atomics, so a run is a pure function of its inputs and --seed (with --seed unset the draws differ '
                        'from run to run: fix the seed to repeat a run)')
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
        for name, default in vars(build_parser().parse_args(["-e", ""])).items():      # a flag's default is build_parser()'s, for any caller's opt
            if not hasattr(opt, name):
                setattr(opt, name, default)
        self.opt, self.log = opt, log
        wide = any(m in "eho" for m in opt.modes)      # the reference's module stops at s, d, y (sr/model.py:119-121)
        self.net = (MuLUTWide if wide else MuLUTInterval if opt.interval in (5, 6) else MuLUT)(opt.expDir, opt.stages, list(opt.modes), upscale=opt.scale, interval=opt.interval,
                                                                                                deterministic=opt.deterministic).cuda()
        if opt.deterministic:
            # one unit of a table sum, as a multiple of the step's largest |grad_out| (include/mulut.h): 2^(ceil(log2(4 sites)) - 60)
            log("{} | deterministic backward: 64-bit fixed-point gradient sums, resolution 2^{} of max |grad_out| per stage call{}".format(
                opt.expDir, math.ceil(math.log2(4 * opt.batchSize * opt.cropSize * opt.cropSize)) - 60,
                "" if opt.seed is not None else " (no --seed: the draws are not fixed)"))
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
        if opt.hostData:
            self.data = CropProvider(opt.trainDir, opt.scale, opt.cropSize, opt.batchSize, opt.seed, opt.makeLR, log)
        else:
            try:      # the set stays on the device for the whole run: at most half of what is free now
                self.data = DeviceCropProvider(opt.trainDir, opt.scale, opt.cropSize, opt.batchSize, opt.seed, max_bytes=torch.cuda.mem_get_info()[0] // 2,
                                               make_lr=opt.makeLR, log=log)
            except TrainingSetTooLarge as e:
                log("{} | training set of {} bytes exceeds half the free device memory ({}): batches are cut on the host".format(opt.expDir, e.nbytes, e.limit))
                self.data = e.host
        if opt.valoutDir is None:
            opt.valoutDir = os.path.join(opt.expDir, "val")
        self.engine, self.engine_at = None, 0
        if opt.valEngine:      # one engine for the run: later installs rewrite its tables in place
            from .engine import MuLUTEngine
            self.engine = MuLUTEngine(next(self.net.parameters()).device.index).configure(opt.stages, opt.modes, opt.scale, opt.interval)
            opt.valEngineResults = {}              # {dataset: [images, 2]} of the last engine validation, for callers
        self.vset = None
        if opt.valResident and os.path.isdir(opt.valDir) and (opt.valStep or self.engine is not None):
            try:      # resident for the whole run: at most a quarter of what is free now
                self.vset = DeviceValSet(opt, max_bytes=torch.cuda.mem_get_info()[0] // 4 if opt.valMaxBytes is None else opt.valMaxBytes, workers=opt.valWorkers)
            except ValidationSetTooLarge as e:
                log("{} | validation set of {} bytes exceeds the {} allowed on the device: validation runs on the host loop".format(opt.expDir, e.nbytes, e.limit))
        # what a validation point runs, and what ends it, chosen here once: from the resident set or on the host loop
        if self.vset is not None:
            self.valid = lambda it: resident_valid_steps(self.net, self.vset, opt, it, log)
            self.engine_valid = lambda it: resident_engine_valid_steps(self.net, self.engine, self.vset, opt, it, log)
            self.close_valid = self.vset.close
        else:
            self.valid = lambda it: valid_steps(self.net, opt, it, log)
            self.engine_valid = lambda it: engine_valid_steps(self.net, self.engine, opt, it, log)
            self.close_valid = lambda: None
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
        if opt.valStep and (i % opt.valStep == 0 or i == 1) and os.path.isdir(opt.valDir):   # :152-158
            t_val = time.time()
            self.valid(i)
            if self.engine is not None:
                opt.valEngineResults, self.engine_at = self.engine_valid(i), i
            self.t_mark += time.time() - t_val

    def finish(self):
        """The last read-back, the engine's score of the tables as they are exported, the export (:162-171); with --valResident every
        PNG is on disk when this returns, and a write that failed is raised here.  Returns the losses."""
        opt, log, net, data, losses = self.opt, self.log, self.net, self.data, self.losses
        losses.extend(self.loss_buf[len(losses):self.i].tolist())
        try:
            if self.engine is not None:
                if self.engine_at != opt.totalIter and os.path.isdir(opt.valDir):      # the tables as they are exported below
                    opt.valEngineResults = self.engine_valid(opt.totalIter)
                self.engine.close()
        finally:
            self.close_valid()
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
