"""Training the SR network on the fused HIP forward and backward (mulut_net_stage_sum / mulut_net_stage_backward of include/mulut.h,
mulut_amd/csrc/mulut_net_train.hip): one NetTrainer per `SRNets` whose parameters live on the device.  With `deterministic=True` the
backward is mulut_net_stage_backward_exact: the input gradient is gathered per pixel in a fixed order instead of added with float
atomics, so every gradient of every stage is a function of the inputs alone, bit for bit.

`stage_sum(stage, x)` is the sum of the 4 M rounded rotation passes of one stage (sr/1_train_model.py:30-35) as one autograd node: the
forward packs the current parameters into the units' weight streams on the device and runs one kernel; the backward runs the
site and weight-gradient kernels per (mode, rotation) pass and hands autograd the gradients of x and of the stage's 12 M parameter
tensors, so `p.grad`, `torch.optim.Adam` and `LambdaLR` work as they do on the torch operators.  `predict` restates `mulut_predict`
(:26-45) over it; the stage's own arithmetic (average, bias, clamp, BPDA round, / 255) stays a few torch element-wise operators.
"""
import torch

from . import _native, network
from .engine import MuLUTError
from .net_engine import NetUnits, _no_gpu, unit_layers

DEFAULT_WS_SITES = 65536      # 173 MB of workspace at nf 64: inside the 256 MB Infinity Cache


def round_func(x):
    """sr/1_train_model.py:48-55: round in the forward, identity in the backward (BPDA)."""
    out = x.clone()
    out.data = torch.round(x).data
    return out


def stage_epilogue(pred, M, last, phase="train"):
    """sr/1_train_model.py:36-43: what follows the sum `pred` of the 4 M passes of a stage."""
    if last:
        x = round_func((pred / M) + 0)
        if phase == "train":
            x = x / 255.0
    else:
        x = round_func(torch.clamp((pred / (M * 4)) + 127, 0, 255)) / 255.0
    return x


class _StageSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, trainer, stage, x, *params):
        ctx.trainer, ctx.stage = trainer, stage
        ctx.versions = [p._version for p in params]      # the units hold THESE parameters: the backward walks the same streams
        ctx.save_for_backward(x)
        return trainer._forward(stage, x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        if [p._version for p in ctx.trainer.stage_params(ctx.stage)] != ctx.versions:
            raise RuntimeError("the parameters of stage %d changed between stage_sum and its backward: the units' weight streams "
                               "no longer hold what the forward ran on" % ctx.stage)
        gx, gp = ctx.trainer._backward(ctx.stage, x, g, ctx.needs_input_grad[2])
        return (None, None, gx) + tuple(gp)


class NetTrainer:
    """Owns a training unit (both weight streams) per `s{stage}_{mode}` module of `model_G`, an `SRNets` on the device.  The units
    follow the parameters: every `stage_sum` packs them anew, on the device.  `ws_sites`: sites per chunk of the backward's workspace,
    which is allocated on first use and kept.  `deterministic`: the backward with the gather-form input gradient (the workspace then
    also holds the tap buffer of a whole pass)."""

    def __init__(self, model_G, ws_sites=DEFAULT_WS_SITES, lib_path=None, deterministic=False):
        _no_gpu()
        self.model = model_G
        p0 = next(model_G.parameters(), None)
        if p0 is None or not p0.is_cuda:
            raise MuLUTError("NetTrainer wants an SRNets on the device (model_G.cuda())")
        self.device = p0.device
        self._units = un = NetUnits(model_G, self.device, True, lib_path)
        self._lib, self.stages, self.modes = un.lib, un.stages, un.modes
        self.ws_sites = int(ws_sites)
        self.deterministic = bool(deterministic)
        self._ws = None
        self.keep_sums = False   # True: last_sums[stage] holds pred of the last stage_sum (tests, logs); off, nothing outlives a step
        self.last_sums = {}

    def close(self):
        if hasattr(self, "_units"):
            self._units.close()

    # -- plumbing ---------------------------------------------------------------------------
    def _stream(self):
        return self._units.stream()

    def _handles(self, stage):
        return self._units.handles(stage)

    def load(self, stage):
        """Pack the current parameters of a stage's units into their streams (stream-ordered, on the device)."""
        self._units.load(stage)

    def stage_params(self, stage):
        """The 12 M parameter tensors of a stage: per mode the six weights, then the six biases."""
        out = []
        for m in self.modes:
            layers = unit_layers(self._units.mods[(stage, m)].model)
            out += [c.weight for c in layers] + [c.bias for c in layers]
        return out

    def _x(self, x, name="x"):
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.is_cuda and x.dim() == 4):
            raise TypeError("%s must be a float32 CUDA tensor [N, C, H, W]" % name)
        if x.device != self.device:
            raise ValueError("%s lives on %s, the module on %s" % (name, x.device, self.device))
        return x.contiguous()

    def workspace(self, stage, sites, min_sites=None):
        """The backward's workspace for chunks of min(sites, ws_sites) sites: kept and grown, never shrunk."""
        chunk = min(sites, self.ws_sites if min_sites is None else min_sites)
        if self.deterministic:      # `sites` is the pass's site count: the tap buffer holds all of them, whatever the chunk
            want = int(self._lib.mulut_net_backward_exact_ws_bytes(self._units.nf(stage), self._units.u(stage), chunk, sites))
        else:
            want = int(self._lib.mulut_net_backward_ws_bytes(self._units.nf(stage), self._units.u(stage), chunk))
        self._units.check(min(want, 0))
        if min_sites is not None:
            return torch.empty(want, dtype=torch.uint8, device=self.device)
        if self._ws is None or self._ws.numel() < want:
            self._ws = torch.empty(want, dtype=torch.uint8, device=self.device)
        return self._ws

    def _forward(self, stage, x):
        x = self._x(x)
        self.load(stage)
        N, C, H, W = x.shape
        u = self._units.u(stage)
        pred = torch.empty((N, C, H * u, W * u), dtype=torch.float32, device=self.device)
        self._units.check(self._lib.mulut_net_stage_sum(self._handles(stage), self.modes.encode(), x.data_ptr(), N, C, H, W, pred.data_ptr(),
                                                        self._stream()))
        if self.keep_sums:
            self.last_sums[stage] = pred.detach()
        return pred

    def _backward(self, stage, x, g, want_gx=True, ws=None):
        """(gx or None, [gradient per tensor of stage_params(stage)]) for g = dL/d(stage_sum).  The units must hold the parameters the
        forward ran on: `_StageSum.backward` raises if a parameter was written since; a direct caller runs `load(stage)` first."""
        x, g = self._x(x), self._x(g, "g")
        N, C, H, W = x.shape
        u = self._units.u(stage)
        if g.shape != (N, C, H * u, W * u):
            raise ValueError("g has the wrong shape")
        ws = self.workspace(stage, N * C * H * W) if ws is None else ws
        if self.deterministic:      # written, not added to
            gx = torch.empty_like(x) if want_gx else None
        else:
            gx = torch.zeros_like(x) if want_gx else None
        params = self.stage_params(stage)
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in params]
        M = len(self.modes)
        gw = _native.ptr_array([grads[12 * m + l] for m in range(M) for l in range(6)])
        gb = _native.ptr_array([grads[12 * m + 6 + l] for m in range(M) for l in range(6)])
        entry = self._lib.mulut_net_stage_backward_exact if self.deterministic else self._lib.mulut_net_stage_backward
        self._units.check(entry(self._handles(stage), self.modes.encode(), x.data_ptr(), g.data_ptr(), N, C, H, W, ws.data_ptr(), ws.numel(),
                                gx.data_ptr() if want_gx else None, gw, gb, self._stream()))
        return gx, grads

    def gx_gather(self, mode, r, t, shape, gx=None):
        """mulut_net_gx_gather for tests: the input gradient of one (pattern, rotation) pass from its tap buffer `t`, float32 [4, ts] on
        the device.  gx None: a new tensor of `shape` = (N, C, H, W) is written; else `gx` is added to, in the order of the definition."""
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_cuda and t.dim() == 2 and t.shape[0] == 4 and t.is_contiguous()):
            raise TypeError("t must be a contiguous float32 CUDA tensor [4, ts]")
        N, C, H, W = shape
        accumulate = gx is not None
        if gx is None:
            gx = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        elif self._x(gx, "gx").data_ptr() != gx.data_ptr() or tuple(gx.shape) != tuple(shape):      # (_x copies what is not contiguous)
            raise ValueError("gx must be contiguous and of `shape`")
        self._units.check(self._lib.mulut_net_gx_gather(self.device.index, mode.encode(), r, t.data_ptr(), t.shape[1], N, C, H, W, gx.data_ptr(),
                                                        int(accumulate), self._stream()))
        return gx

    # -- compute ------------------------------------------------------------------------------
    def stage_sum(self, stage, x):
        """float32 [N, C, H u, W u]: pred of sr/1_train_model.py:30-35 for one stage, differentiable in x and the stage's parameters."""
        stage = int(stage)
        return _StageSum.apply(self, stage, x, *self.stage_params(stage))

    def predict(self, x, phase="train"):
        """`mulut_predict(model_G, x, phase, opt)` of sr/1_train_model.py:26-45."""
        for s in range(1, self.stages + 1):
            x = stage_epilogue(self.stage_sum(s, x), len(self.modes), s == self.stages, phase)
        return x


def torch_predict(model_G, x, modes, stages, phase="train"):
    """The same on `network.SRNets` as torch operators: sr/1_train_model.py:26-45 line for line."""
    import torch.nn.functional as F
    for s in range(stages):
        pred = 0
        for mode in modes:
            pad = network.TAPS[mode.upper()][0] - 1
            for r in [0, 1, 2, 3]:
                pred = pred + round_func(torch.rot90(model_G(F.pad(torch.rot90(x, r, [2, 3]), (0, pad, 0, pad), mode='replicate'),
                                                             stage=s + 1, mode=mode), (4 - r) % 4, [2, 3]) * 127)
        x = stage_epilogue(pred, len(modes), s + 1 == stages, phase)
    return x


def step_flops(nf, scale, modes, stages, batch, crop):
    """FLOPs of the arithmetic one training step needs: 3 x the forward's multiply-adds x 2 (forward, backward-data, weight gradient;
    the backward's recompute of the forward is overhead, not counted)."""
    total = 0
    for s in range(1, stages + 1):
        u = scale if s == stages else 1
        macs = 4 * nf + nf * nf * 10 + 5 * nf * u * u
        total += 4 * len(modes) * batch * crop * crop * macs      # every stage before the last keeps the size
    return 3 * 2 * total

