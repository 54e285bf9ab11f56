"""GPU twin of the reference's differentiable LUT module (SURVEY.md 8b "Python callable 2").

``MuLUT(lut_folder, stages, modes, upscale=4, interval=4)`` keeps the reference's constructor, parameter
names (``weight_s{stage}_{mode}``, float32 [83521, u*u] = int8/127, sr/model.py:49-57) and forward contract
(x float32 [B,C,H,W] in 0..1 -> [B,C,H*u,W*u] in 0..1, :289-312), so ``sr/3_finetune_lut.py`` can train it with
the same Adam / cosine schedule and write ``LUT_ft_*.npy`` the same way (:162-169).  Each stage runs as one
forward and one backward HIP kernel through the C ABI (mulut_ft_wide_stage_forward / _backward, for every class here); torch provides autograd
plumbing, parameters and the optimiser only.  ``MuLUTInterval`` is the same module at intervals 5 and 6, ``MuLUTWide`` the one
for mode lists with the 4 x 4 patterns e, h, o (intervals 4, 5 and 6).
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

from . import _native
from ._native import ptr_array, stream_ptr


class _StageFn(torch.autograd.Function):
    """One stage: all modes x 4 rotations, per-pass BPDA rounding, clamp/round of the stage output."""

    @staticmethod
    def forward(ctx, x, modes, is_last, u, interval, *weights):
        # the kernels take raw pointers: a tensor of another type or on another device would be read as float32 levels at an address
        # of this device, so it is refused here, before any library call (as MuLUTEngine._dev_u8 refuses for inference)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            raise TypeError("x must be a float32 CUDA tensor [B, C, H, W] (got {} on {})".format(
                getattr(x, "dtype", type(x).__name__), getattr(x, "device", "the host")))
        for w in weights:
            if w.device != x.device:
                raise ValueError("a table lives on {}, x on {}".format(w.device, x.device))
        lib = _native.load()
        x = x.contiguous()
        stream = stream_ptr(x.device)
        # weight = clamp(round_func(weight * 127), -127, 127)       sr/model.py:74-76, the stage's tables in one launch
        ws = [w.detach().contiguous() for w in weights]
        n = ws[0].numel()
        if any(w.numel() != n or w.dtype != torch.float32 for w in ws):
            raise ValueError("the tables of a stage must be float32 of one shape")
        wq_all = torch.empty((len(ws), n), dtype=torch.float32, device=x.device)
        wq = [wq_all[m].view(w.shape) for m, w in enumerate(ws)]
        _native.check(lib.mulut_ft_quantize(x.device.index, ptr_array(ws), ptr_array(wq), len(ws), n, stream))
        B, C, H, W = x.shape
        out = torch.empty((B, C, H * u, W * u), dtype=torch.float32, device=x.device)
        # where the stage's clamp passes gradient, 16 bits per site: saves the backward a recomputation of the stage forward
        inside = torch.empty((B, C, H, W), dtype=torch.int16, device=x.device)
        # any list over s, d, y, e, h, o at interval 4, 5 or 6: for a list of s, d, y the launches of the narrow entry points
        rc = lib.mulut_ft_wide_stage_forward(x.device.index, int(interval), ptr_array(wq), modes.encode(), int(is_last), int(u),
                                             x.data_ptr(), B, C, H, W, out.data_ptr(), inside.data_ptr(), stream)
        if rc == -2:      # MULUT_EMODE: the reference's ValueError("Mode {} not implemented.")
            raise ValueError(lib.mulut_strerror(rc).decode())
        _native.check(rc)
        ctx.save_for_backward(x, wq_all, inside, *ws)
        ctx.cfg = (modes, is_last, u, interval)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _native.load()
        modes, is_last, u, interval = ctx.cfg
        x, wq_all, inside, *ws = ctx.saved_tensors
        wq = [wq_all[m].view(w.shape) for m, w in enumerate(ws)]
        gout = gout.contiguous()
        B, C, H, W = x.shape
        g_all = torch.zeros_like(wq_all)
        gwq = [g_all[m].view(w.shape) for m, w in enumerate(ws)]
        gx = torch.zeros_like(x)
        stream = stream_ptr(x.device)
        if getattr(ctx, "exact", False):
            # fixed-point sums (mulut_ft_exact_stage_backward): the same bits whatever order the hardware runs the waves in.  The
            # workspace comes from torch's allocator on the current stream, so its reuse is ordered behind this call.
            need = _native.check(lib.mulut_ft_exact_ws_bytes(int(interval), modes.encode(), int(u), B, C, H, W))
            work = torch.empty(need // 8, dtype=torch.int64, device=x.device)
            _native.check(lib.mulut_ft_exact_stage_backward(x.device.index, int(interval), ptr_array(wq), modes.encode(), int(is_last), int(u),
                                                            x.data_ptr(), gout.data_ptr(), inside.data_ptr(), B, C, H, W, ptr_array(gwq),
                                                            gx.data_ptr(), work.data_ptr(), need, stream))
        else:
            _native.check(lib.mulut_ft_wide_stage_backward(x.device.index, int(interval), ptr_array(wq), modes.encode(), int(is_last), int(u),
                                                           x.data_ptr(), gout.data_ptr(), inside.data_ptr(), B, C, H, W, ptr_array(gwq),
                                                           gx.data_ptr(), stream))
        # backward of clamp(round_func(w*127)): round is identity (BPDA), clamp passes inside [-127,127], x127 -- in place, one launch
        _native.check(lib.mulut_ft_quantize_backward(x.device.index, ptr_array(ws), ptr_array(gwq), len(ws), ws[0].numel(), stream))
        return (gx, None, None, None, None) + tuple(gwq)


class _StageFnExact(_StageFn):
    """The same stage with the bit-reproducible backward (``deterministic=True``): quantise, forward, mask and quantise-backward are
    _StageFn's; the table and input gradients are summed in 64-bit fixed point (mulut_ft_exact_stage_backward)."""

    @staticmethod
    def forward(ctx, *args):
        ctx.exact = True
        return _StageFn.forward(ctx, *args)


class MuLUT(nn.Module):
    """PyTorch module for LUT-aware fine-tuning on the GPU (twin of sr/model.py:39-312), sampling interval 4.
    Intervals 5 and 6 are ``MuLUTInterval``; mode lists with e, h or o are ``MuLUTWide``.
    ``deterministic=True``: the backward sums every gradient in 64-bit fixed point instead of with float32 atomics -- the same bits
    on every run (torch's ``use_deterministic_algorithms`` for this module; resolution and cost: DESIGN.md section 8)."""

    MODES = "sdy"       # the patterns the class takes

    def __init__(self, lut_folder, stages, modes, upscale=4, interval=4, deterministic=False):
        super().__init__()
        self._check_interval(interval)
        self.deterministic = bool(deterministic)
        self.interval, self.upscale, self.stages = interval, upscale, stages
        self.modes = "".join(modes)
        for mode in self.modes:
            # this class and MuLUTInterval keep to the reference module's s, d and y (the 4 x 4 patterns e, h, o are MuLUTWide);
            # the reference raises the same way for any mode it does not implement (sr/model.py:121)
            if mode not in self.MODES:
                raise ValueError("Mode {} not implemented.".format(mode))
        for s in range(stages):
            stage = s + 1
            scale = upscale if stage == stages else 1
            for mode in self.modes:
                # writer-side naming, as the reference's module reads it (sr/model.py:51-53)
                path = os.path.join(lut_folder, "LUT_x{}_{}bit_int8_s{}_{}.npy".format(upscale, interval, stage, mode))
                arr = np.load(path).reshape(-1, scale * scale).astype(np.float32) / 127.0
                self.register_parameter("weight_s{}_{}".format(stage, mode), nn.Parameter(torch.from_numpy(arr)))

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("mulut_amd.finetune.{} has no CPU path; move the module and input to the GPU".format(type(self).__name__))
        x = x * 255.0
        for s in range(self.stages):
            stage = s + 1
            last = stage == self.stages
            weights = [getattr(self, "weight_s{}_{}".format(stage, m)) for m in self.modes]
            x = (_StageFnExact if self.deterministic else _StageFn).apply(x, self.modes, last, self.upscale if last else 1, self.interval, *weights)
        return x / 255.0

    @staticmethod
    def _check_interval(interval):
        if interval != 4:
            # this class runs the kernels of mulut_ft.hip, built for q = 16, L = 17
            raise NotImplementedError("mulut_amd.finetune.MuLUT: fine-tuning is interval-4 only (got interval {}); "
                                      "intervals 5 and 6 are mulut_amd.finetune.MuLUTInterval".format(interval))

    def install_into(self, engine):
        """The current parameters into a MuLUTEngine of the same configuration, as the tables export_int8() writes into the
        LUT_ft files (sr/3_finetune_lut.py:162-169): the engine then runs the cascade users deploy on what the module holds now."""
        mine = (self.stages, self.modes, self.upscale, self.interval)
        theirs = (engine.stages, engine.modes, engine.scale, engine.interval)
        if mine != theirs:
            raise ValueError("engine configured as (stages, modes, scale, interval) = {}, module is {}".format(theirs, mine))
        return engine.set_lut_dict(self.export_int8())

    def export_int8(self):
        """{ 's{stage}_{mode}': int8 table } as sr/3_finetune_lut.py:162-169 writes LUT_ft_*.npy."""
        out = {}
        for s in range(self.stages):
            for m in self.modes:
                w = getattr(self, "weight_s{}_{}".format(s + 1, m)).detach().cpu().numpy()
                out["s{}_{}".format(s + 1, m)] = np.round(np.clip(w, -1, 1) * 127).astype(np.int8)
        return out


class MuLUTInterval(MuLUT):
    """The same module at the sampling intervals 5 and 6 (the reference's ``MuLUT(..., interval=5 | 6)``, sr/model.py:42-44):
    tables of 6,561 / 625 rows, read from ``LUT_x{scale}_{interval}bit_int8_s{stage}_{mode}.npy`` as transfer_to_lut writes them;
    the stages run on the kernels of mulut_amd/csrc/mulut_ft_interval.hip."""

    def __init__(self, lut_folder, stages, modes, upscale=4, interval=5, deterministic=False):
        super().__init__(lut_folder, stages, modes, upscale=upscale, interval=interval, deterministic=deterministic)

    @staticmethod
    def _check_interval(interval):
        if interval not in (5, 6):
            raise ValueError("mulut_amd.finetune.MuLUTInterval takes interval 5 or 6 (got {}); interval 4 is "
                             "mulut_amd.finetune.MuLUT".format(interval))


class MuLUTWide(MuLUT):
    """The same module for any list over the six sampling patterns s, d, y, e, h, o, at interval 4, 5 or 6.  The reference's
    module ends its pattern cascade at s, d, y with "more sampling modes can be implemented similarly" (sr/model.py:119-121) while
    its network and trainer define all six (common/network.py:173-215): this class fine-tunes the tables transfer_to_lut writes
    for them, same file names, parameter names and forward contract.  The backward kernels stage a 3-pixel halo of the input
    gradient when the list holds e, h or o, and are exactly what ``MuLUT`` / ``MuLUTInterval`` run when it does not."""

    MODES = "sdyeho"

    @staticmethod
    def _check_interval(interval):
        if interval not in (4, 5, 6):
            raise ValueError("mulut_amd.finetune.MuLUTWide takes interval 4, 5 or 6 (got {})".format(interval))


class Adam(torch.optim.Optimizer):
    """The reference's optimiser (sr/3_finetune_lut.py:86: torch.optim.Adam with L2 weight decay, no amsgrad) as one HIP launch over
    every table of a parameter group (mulut_ft_adam): float32 parameters and moments, the step's arithmetic in float64 -- each stored
    value is the float64 Adam's rounded once.  State as torch's: ``state[p]`` holds ``step`` (a float32 scalar on the host),
    ``exp_avg`` and ``exp_avg_sq``; learning-rate schedulers drive ``param_groups[..]['lr']`` as they do torch's."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid Adam setting: lr {}, betas {}, eps {}, weight_decay {}".format(lr, betas, eps, weight_decay))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _native.load()
        for group in self.param_groups:
            by_step = {}      # (device, number of the step) -> parameters: one launch each (one in all for a module's tables)
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.dtype == torch.float32 and p.grad.device == p.device):
                    raise TypeError("mulut_amd.finetune.Adam steps contiguous float32 CUDA parameters with float32 gradients on their device")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                by_step.setdefault((p.device, int(st["step"].item())), []).append(p)
            for (device, step), ps in by_step.items():
                grads = [p.grad.contiguous() for p in ps]
                n = (ctypes.c_longlong * len(ps))(*[p.numel() for p in ps])
                _native.check(lib.mulut_ft_adam(device.index, ptr_array(ps), ptr_array(grads), ptr_array([self.state[p]["exp_avg"] for p in ps]),
                                                ptr_array([self.state[p]["exp_avg_sq"] for p in ps]), n, len(ps), step, float(group["lr"]),
                                                group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"],
                                                stream_ptr(device)))
        return loss
