"""The trained network on the fused HIP forward (mulut_net_* of include/mulut.h, mulut_amd/csrc/mulut_net.hip): one NetEngine per
`SRNets`, one device unit per `s{stage}_{mode}` module.

What `network.SRNets` computes as a chain of torch operators with a [sites, 5 * nf] activation matrix per layer runs here as one kernel
per call with the activations in registers: a table of sr/2_transfer_to_lut.py, one rotation pass, one stage or the whole cascade of
sr/1_train_model.py's `mulut_predict(..., 'valid')`, bytes to bytes.  torch is used for device memory and streams only.
"""
import ctypes
import re

import numpy as np
import torch

from . import _native, network
from .engine import MuLUTError
from .lut_io import lut_rows

_MODULE = re.compile(r"^s(\d+)_([a-z])$")


def _dev(t, dtype, name):
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_cuda and t.is_contiguous()):
        raise TypeError("%s must be a contiguous %s CUDA tensor" % (name, str(dtype).replace("torch.", "")))
    return t


def unit_layers(unit):
    """The six convolutions of a dense MuLUTUnit, conv1..conv6."""
    if not isinstance(unit.conv2, network.DenseConv):
        raise MuLUTError("mulut error -5: only dense=True units run on the fused forward")
    return [unit.conv1.conv] + [c.conv1.conv for c in (unit.conv2, unit.conv3, unit.conv4, unit.conv5)] + [unit.conv6.conv]


def layer_shapes(nf, u):
    """(out, in) of conv1..conv6 of a dense unit: net_layer_out / net_layer_in of csrc/mulut_net.h."""
    return [(u * u if L == 6 else nf, 4 if L == 1 else (L - 1) * nf) for L in range(1, 7)]


def discover(model_G, need_bias=False):
    """The `s{stage}_{mode}` units of an `SRNets`, validated; needs no GPU and no library.  Returns (mods, stages, modes, shape):
    mods[(stage, mode)] is the SRNet, modes the letters of stage 1 in the module's own order (the order they were added in), which
    every stage must hold, and shape[(stage, mode)] = (nf, u) of a unit whose six layers are those of a dense unit.  A layer without a
    bias is refused if `need_bias` (training) and otherwise read as zeros."""
    mods = {}
    for name, mod in model_G.named_children():
        m = _MODULE.match(name)
        if m and isinstance(getattr(mod, "model", None), network.MuLUTUnit):
            mods[(int(m.group(1)), m.group(2))] = mod
    if not mods:
        raise MuLUTError("no s{stage}_{mode} module found: the network is to be an SRNets")
    stages = max(s for s, _ in mods)
    modes = "".join(m for s, m in mods if s == 1)
    for s in range(1, stages + 1):
        if "".join(m for t, m in mods if t == s) != modes:
            raise MuLUTError("stage %d does not hold the modes %r of stage 1" % (s, modes))
    shape = {}
    for key, mod in mods.items():
        layers = unit_layers(mod.model)
        nf, u = int(layers[0].out_channels), int(mod.model.upscale)
        got = [(c.weight.shape[0], c.weight[0].numel()) for c in layers]
        if got != layer_shapes(nf, u):
            raise MuLUTError("mulut error -4: layer shapes %r of %s are not those of a dense unit, %r" % (got, mod.mode, layer_shapes(nf, u)))
        if need_bias and any(c.bias is None for c in layers):
            raise MuLUTError("mulut error -4: a layer of %s has no bias: training wants a dense unit with biases" % mod.mode)
        shape[key] = (nf, u)
    return mods, stages, modes, shape


def unit_param_pointers(unit, device):
    """(w[6], b[6]) as ctypes arrays of device pointers for mulut_net_unit_load_dev, and the tensors that must outlive the launch."""
    ws, bs = [], []
    for c in unit_layers(unit):
        ws.append(c.weight.detach().to(device=device, dtype=torch.float32).contiguous())
        bs.append((c.bias.detach() if c.bias is not None else torch.zeros(c.weight.shape[0])).to(device=device, dtype=torch.float32).contiguous())
    return _native.ptr_array(ws), _native.ptr_array(bs), ws + bs


class NetUnits:
    """The `mulut_net_unit` handles of `discover(model_G)` on `device`, under NetEngine and NetTrainer.  train False: each unit is
    created from the module's weights as they are now, packed on the host (mulut_net_unit_create); True: both streams, zeroed
    (mulut_net_unit_create_train), to be filled by `load`."""

    def __init__(self, model_G, device, train=False, lib_path=None):
        self._h = {}
        self.mods, self.stages, self.modes, self.shape = discover(model_G, train)
        self.lib, self.device = _native.load(lib_path), device
        try:
            for key, mod in self.mods.items():
                self._h[key] = self._create(mod.model, *self.shape[key], train)
        except Exception:
            self.close()
            raise

    def check(self, rc):
        return _native.check(rc, MuLUTError)

    def _create(self, unit, nf, u, train):
        h = ctypes.c_void_p()
        if train:
            self.check(self.lib.mulut_net_unit_create_train(self.device.index, nf, u, ctypes.byref(h)))
            return h
        layers, fp = unit_layers(unit), ctypes.POINTER(ctypes.c_float)
        ws = [np.ascontiguousarray(c.weight.detach().cpu().numpy().reshape(c.weight.shape[0], -1), dtype=np.float32) for c in layers]
        bs = [np.ascontiguousarray((c.bias.detach().cpu().numpy() if c.bias is not None else np.zeros(c.weight.shape[0])), dtype=np.float32)
              for c in layers]
        wp = (fp * 6)(*[w.ctypes.data_as(fp) for w in ws])
        bp = (fp * 6)(*[b.ctypes.data_as(fp) for b in bs])
        self.check(self.lib.mulut_net_unit_create(self.device.index, nf, u, wp, bp, ctypes.byref(h)))
        return h

    def close(self):
        for h in self._h.values():
            self.lib.mulut_net_unit_destroy(h)
        self._h = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self):
        return _native.stream_ptr(self.device)

    def nf(self, stage):
        return self.shape[(stage, self.modes[0])][0]

    def u(self, stage):
        return self.shape[(stage, self.modes[0])][1]

    def handle(self, stage, mode):
        try:
            return self._h[(int(stage), mode)]
        except KeyError:
            raise ValueError("Mode {} not implemented.".format(mode)) from None

    def handles(self, stage):
        """The units of a stage in the order of `modes`, as the stage calls take them."""
        return (ctypes.c_void_p * len(self.modes))(*[self.handle(stage, m).value for m in self.modes])

    def load(self, stage, model_G=None):
        """Pack the current parameters of a stage's modules -- those of `model_G`, a module tree like the one the units were made
        from, if given -- into the units' streams through the device pack, mulut_net_unit_load_dev: one small launch per unit on the
        current stream, no host round trip for parameters that live on the device."""
        for m in self.modes:
            mod = self.mods[(stage, m)] if model_G is None else getattr(model_G, "s{}_{}".format(stage, m))
            wp, bp, keep = unit_param_pointers(mod.model, self.device)
            self.check(self.lib.mulut_net_unit_load_dev(self.handle(stage, m), wp, bp, self.stream()))
            del keep      # (stream-ordered: torch's allocator does not hand the memory out to another stream)


def _no_gpu():
    if not torch.cuda.is_available():
        raise MuLUTError("no GPU visible: mulut_amd has no CPU path")


class NetPlan:
    """Owns a `mulut_net_plan` of a NetEngine: a list of images of different sizes through the whole cascade, HWC bytes in one device
    pool to HWC bytes in another, in `stages` launches (csrc/mulut_net_list.hip).  The units stay the engine's: `load_weights` there
    is seen by the next `run`, and the engine must outlive the plan."""

    def __init__(self, engine, items, ch=3):
        rows = [tuple(int(v) for v in it) for it in items]
        if any(len(r) != 6 for r in rows):
            raise ValueError("an item is (in_off, out_off, h, w, in_pool_bytes, out_pool_bytes)")
        self._engine, self._lib, self._h = engine, engine._lib, None
        self.n, self.ch = len(rows), int(ch)
        self.in_bytes, self.out_bytes = max((r[4] for r in rows), default=0), max((r[5] for r in rows), default=0)
        table = np.zeros((max(self.n, 1), 5), np.int64)      # mulut_net_item: in_off, out_off, (h, w) as two int32, the two pool sizes
        for k, (in_off, out_off, h, w, in_pool, out_pool) in enumerate(rows):
            if not (-2 ** 31 <= h < 2 ** 31 and -2 ** 31 <= w < 2 ** 31):
                raise ValueError("item %d: h and w are 32-bit" % k)
            table[k, 0], table[k, 1], table[k, 3], table[k, 4] = in_off, out_off, in_pool, out_pool
            table[k, 2:3].view(np.int32)[:] = (h, w)
        plan = ctypes.c_void_p()
        engine._check(self._lib.mulut_net_plan_create(engine.device.index, table.ctypes.data, self.n, self.ch, engine.stages, engine.scale,
                                                      ctypes.byref(plan)))
        self._h = plan
        un = engine._units
        self._handles = (ctypes.c_void_p * (engine.stages * len(engine.modes)))(
            *[un.handle(s, m).value for s in range(1, engine.stages + 1) for m in engine.modes])

    def _pool(self, t, nbytes, name):
        _dev(t, torch.uint8, name)
        if t.device != self._engine.device:
            raise ValueError("%s lives on %s, engine on %s" % (name, t.device, self._engine.device))
        if t.numel() < nbytes:
            raise ValueError("%s holds %d bytes, the items stated %d" % (name, t.numel(), nbytes))
        return t.data_ptr()

    def run(self, in_pool, out_pool):
        """`stages` launches on torch's current stream, nothing else: capturable.  Runs of one plan are to be ordered one behind the other."""
        if self._h is None:
            raise MuLUTError("the plan is closed")
        e = self._engine
        e._check(self._lib.mulut_net_plan_run(self._h, self._handles, e.modes.encode(), self._pool(in_pool, self.in_bytes, "in_pool"),
                                              self._pool(out_pool, self.out_bytes, "out_pool"), e._stream()))
        return out_pool

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.mulut_net_plan_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NetEngine:
    """Owns a `mulut_net_unit` per module of `model_G` (an `SRNets`, also one rebuilt by `network.load_checkpoint`).  The weights are
    read once, here: a later change of the module's parameters is not seen until `load_weights` packs them anew, on the device.  Every method takes and returns device tensors and
    queues its work on torch's current stream."""

    def __init__(self, model_G, device=0, lib_path=None):
        _no_gpu()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self._units = un = NetUnits(model_G, self.device, False, lib_path)
        self._lib, self.stages, self.modes = un.lib, un.stages, un.modes
        if any(un.shape[(s, m)][1] != un.u(s) for s, m in un.shape):
            self.close()
            raise MuLUTError("mulut error -4: the units of a stage differ in upscale")
        self.scale = int(np.prod([un.u(s) for s in range(1, self.stages + 1)]))

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc):
        self._units.check(rc)

    def load_weights(self, model_G):
        """Refresh every unit from the current parameters of `model_G` (the module tree this engine was built from), on the device."""
        for s in range(1, self.stages + 1):
            self._units.load(s, model_G)
        return self

    def close(self):
        if hasattr(self, "_units"):
            self._units.close()

    def _stream(self):
        return self._units.stream()

    def upscale(self, stage):
        return self._units.u(int(stage))

    def _u8(self, x, name="x_u8"):
        _dev(x, torch.uint8, name)
        if x.device != self.device:
            raise ValueError("%s lives on %s, engine on %s" % (name, x.device, self.device))
        if x.dim() != 4:
            raise ValueError("%s must be planar [N, C, H, W]" % name)
        return x

    # -- compute ------------------------------------------------------------------------------
    def table(self, stage, mode, interval=4):
        """int8 [L^4, 1, u, u] on the device: the table sr/2_transfer_to_lut.py:86-109 makes of this module."""
        h, u = self._units.handle(stage, mode), self.upscale(stage)
        if interval not in (4, 5, 6):
            self._check(-5)
        out = torch.empty((lut_rows(interval), 1, u, u), dtype=torch.int8, device=self.device)
        self._check(self._lib.mulut_net_table(h, int(interval), out.data_ptr(), self._stream()))
        return out

    def pass_(self, stage, mode, r, x_u8):
        """int8 [N, C, H*u, W*u]: one (mode, rotation) term of sr/1_train_model.py:33-35, round(127 * net(...)) rotated back."""
        h, u = self._units.handle(stage, mode), self.upscale(stage)
        x = self._u8(x_u8)
        N, C, H, W = x.shape
        out = torch.empty((N, C, H * u, W * u), dtype=torch.int8, device=self.device)
        self._check(self._lib.mulut_net_pass(h, mode.encode()[:1], int(r), x.data_ptr(), N, C, H, W, out.data_ptr(), self._stream()))
        return out

    def stage(self, stage, x_u8, out=None):
        """uint8 [N, C, H*u, W*u]: one stage of mulut_predict in the 'valid' phase (sr/1_train_model.py:29-43)."""
        stage = int(stage)
        handles, u = self._units.handles(stage), self.upscale(stage)
        x = self._u8(x_u8)
        N, C, H, W = x.shape
        if out is None:
            out = torch.empty((N, C, H * u, W * u), dtype=torch.uint8, device=self.device)
        elif self._u8(out, "out").shape != (N, C, H * u, W * u):
            raise ValueError("out has the wrong shape")
        self._check(self._lib.mulut_net_stage(handles, self.modes.encode(), int(stage == self.stages), x.data_ptr(), out.data_ptr(),
                                              N, C, H, W, self._stream()))
        return out

    def plan(self, items, ch=3):
        """A NetPlan over `items`, each (in_off, out_off, h, w, in_pool_bytes, out_pool_bytes): image k is uint8 [h][w][ch] at byte
        in_off of the input pool, and its result -- `predict` of that image alone, permuted to HWC -- goes to byte out_off of the
        output pool as uint8 [h * scale][w * scale][ch].  `run(in_pool, out_pool)` is `stages` launches on the current stream."""
        return NetPlan(self, items, ch)

    def predict(self, x_u8):
        """The whole cascade, bytes to bytes: np.round(np.clip(mulut_predict(model_G, x / 255, 'valid', opt), 0, 255)) of
        sr/1_train_model.py:93-101."""
        x = self._u8(x_u8)
        for s in range(1, self.stages + 1):
            x = self.stage(s, x)
        return x
