"""Training the SR network on the fused HIP forward and backward (mulut_net_stage_sum / mulut_net_stage_backward of include/mulut.h,
mulut_amd/csrc/mulut_net_train.hip): one NetTrainer per `SRNets` whose parameters live on the device.

`stage_sum(stage, x)` is the sum of the 4 M rounded rotation passes of one stage (sr/1_train_model.py:30-35) as one autograd node: the
forward packs the current parameters into the units' weight streams on the device and runs one kernel; the backward runs the
site and weight-gradient kernels per (mode, rotation) pass and hands autograd the gradients of x and of the stage's 12 M parameter
tensors, so `p.grad`, `torch.optim.Adam` and `LambdaLR` work as they do on the torch operators.  `predict` restates `mulut_predict`
(:26-45) over it; the stage's own arithmetic (average, bias, clamp, BPDA round, / 255) stays a few torch element-wise operators.
"""
import ctypes

import torch

from . import _native
from .engine import MuLUTError
from .net_engine import _MODULE, unit_layers, unit_param_pointers
from . import network

DEFAULT_WS_SITES = 65536      # 173 MB of workspace at nf 64: inside the 256 MB Infinity Cache


def round_func(x):
    """sr/1_train_model.py:48-55: round in the forward, identity in the backward (BPDA)."""
    out = x.clone()
    out.data = torch.round(x).data
    return out


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
    which is allocated on first use and kept."""

    def __init__(self, model_G, ws_sites=DEFAULT_WS_SITES, lib_path=None):
        self._lib = _native.load(lib_path)
        self._units = {}
        if not torch.cuda.is_available():
            raise MuLUTError("no GPU visible: mulut_amd has no CPU path")
        self.model = model_G
        found = {}
        for name, mod in model_G.named_children():
            m = _MODULE.match(name)
            if m and isinstance(getattr(mod, "model", None), network.MuLUTUnit):
                found[(int(m.group(1)), m.group(2))] = mod
        if not found:
            raise MuLUTError("no s{stage}_{mode} module found: NetTrainer wants an SRNets")
        p0 = next(model_G.parameters())
        if not p0.is_cuda:
            raise MuLUTError("NetTrainer wants the module on the device (model_G.cuda())")
        self.device = p0.device
        self.stages = max(s for s, _ in found)
        self.modes = "".join(m for s, m in found if s == 1)
        for s in range(1, self.stages + 1):
            if "".join(m for t, m in found if t == s) != self.modes:
                raise MuLUTError("stage %d does not hold the modes %r of stage 1" % (s, self.modes))
        self._mods = found
        self.ws_sites = int(ws_sites)
        self._ws = None
        self.keep_sums = False   # True: last_sums[stage] holds pred of the last stage_sum (tests, logs); off, nothing outlives a step
        self.last_sums = {}
        self._nf, self._u = {}, {}
        try:
            for (s, mode), mod in found.items():
                layers = unit_layers(mod.model)
                nf, u = int(layers[0].out_channels), int(mod.model.upscale)
                want = [(nf, 4)] + [(nf, nf * k) for k in (1, 2, 3, 4)] + [(u * u, 5 * nf)]
                if [(c.weight.shape[0], c.weight[0].numel()) for c in layers] != want or any(c.bias is None for c in layers):
                    raise MuLUTError("mulut error -4: the layers of %s are not those of a dense unit with biases" % mod.mode)
                h = ctypes.c_void_p()
                _native.check(self._lib.mulut_net_unit_create_train(self.device.index, nf, u, ctypes.byref(h)), MuLUTError)
                self._units[(s, mode)] = h
                self._nf[s], self._u[s] = nf, u
        except Exception:
            self.close()
            raise

    def close(self):
        for h in getattr(self, "_units", {}).values():
            self._lib.mulut_net_unit_destroy(h)
        self._units = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing ---------------------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _handles(self, stage):
        return (ctypes.c_void_p * len(self.modes))(*[self._units[(stage, m)].value for m in self.modes])

    def stage_params(self, stage):
        """The 12 M parameter tensors of a stage: per mode the six weights, then the six biases."""
        out = []
        for m in self.modes:
            layers = unit_layers(self._mods[(stage, m)].model)
            out += [c.weight for c in layers] + [c.bias for c in layers]
        return out

    def _x(self, x, name="x"):
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.is_cuda and x.dim() == 4):
            raise TypeError("%s must be a float32 CUDA tensor [N, C, H, W]" % name)
        if x.device != self.device:
            raise ValueError("%s lives on %s, the module on %s" % (name, x.device, self.device))
        return x.contiguous()

    def load(self, stage):
        """Pack the current parameters of a stage's units into their streams (stream-ordered, on the device)."""
        for m in self.modes:
            wp, bp, keep = unit_param_pointers(self._mods[(stage, m)].model, self.device)
            _native.check(self._lib.mulut_net_unit_load_dev(self._units[(stage, m)], wp, bp, self._stream()), MuLUTError)
            del keep

    def workspace(self, stage, sites, min_sites=None):
        """The backward's workspace for chunks of min(sites, ws_sites) sites: kept and grown, never shrunk."""
        want = int(self._lib.mulut_net_backward_ws_bytes(self._nf[stage], self._u[stage], min(sites, self.ws_sites if min_sites is None else min_sites)))
        _native.check(min(want, 0), MuLUTError)
        if min_sites is not None:
            return torch.empty(want, dtype=torch.uint8, device=self.device)
        if self._ws is None or self._ws.numel() < want:
            self._ws = torch.empty(want, dtype=torch.uint8, device=self.device)
        return self._ws

    def _forward(self, stage, x):
        x = self._x(x)
        self.load(stage)
        N, C, H, W = x.shape
        u = self._u[stage]
        pred = torch.empty((N, C, H * u, W * u), dtype=torch.float32, device=self.device)
        _native.check(self._lib.mulut_net_stage_sum(self._handles(stage), self.modes.encode(), x.data_ptr(), N, C, H, W, pred.data_ptr(),
                                                    self._stream()), MuLUTError)
        if self.keep_sums:
            self.last_sums[stage] = pred.detach()
        return pred

    def _backward(self, stage, x, g, want_gx=True, ws=None):
        """(gx or None, [gradient per tensor of stage_params(stage)]) for g = dL/d(stage_sum).  The units must hold the parameters the
        forward ran on: `_StageSum.backward` raises if a parameter was written since; a direct caller runs `load(stage)` first."""
        x, g = self._x(x), self._x(g, "g")
        N, C, H, W = x.shape
        u = self._u[stage]
        if g.shape != (N, C, H * u, W * u):
            raise ValueError("g has the wrong shape")
        ws = self.workspace(stage, N * C * H * W) if ws is None else ws
        gx = torch.zeros_like(x) if want_gx else None
        params = self.stage_params(stage)
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in params]
        M = len(self.modes)
        gw = (ctypes.c_void_p * (6 * M))(*[grads[12 * m + l].data_ptr() for m in range(M) for l in range(6)])
        gb = (ctypes.c_void_p * (6 * M))(*[grads[12 * m + 6 + l].data_ptr() for m in range(M) for l in range(6)])
        _native.check(self._lib.mulut_net_stage_backward(self._handles(stage), self.modes.encode(), x.data_ptr(), g.data_ptr(), N, C, H, W,
                                                         ws.data_ptr(), ws.numel(), gx.data_ptr() if want_gx else None, gw, gb,
                                                         self._stream()), MuLUTError)
        return gx, grads

    # -- compute ------------------------------------------------------------------------------
    def stage_sum(self, stage, x):
        """float32 [N, C, H u, W u]: pred of sr/1_train_model.py:30-35 for one stage, differentiable in x and the stage's parameters."""
        stage = int(stage)
        return _StageSum.apply(self, stage, x, *self.stage_params(stage))

    def predict(self, x, phase="train"):
        """`mulut_predict(model_G, x, phase, opt)` of sr/1_train_model.py:26-45."""
        M = len(self.modes)
        for s in range(1, self.stages + 1):
            pred = self.stage_sum(s, x)
            if s == self.stages:
                x = round_func(pred / M + 0)
                if phase == "train":
                    x = x / 255.0
            else:
                x = round_func(torch.clamp(pred / (M * 4) + 127, 0, 255)) / 255.0
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
        if s + 1 == stages:
            x = round_func((pred / len(modes)) + 0)
            if phase == "train":
                x = x / 255.0
        else:
            x = round_func(torch.clamp((pred / (len(modes) * 4)) + 127, 0, 255)) / 255.0
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

