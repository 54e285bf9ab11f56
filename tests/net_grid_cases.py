"""What tests/test_net_grid_cpu.py and tests/test_gpu_net_grid.py share: models that reach every compiled (MT, U) instance of the fused
network kernels, the smallest shapes at which a site body can go wrong, and a comparison that holds a kernel value EXACTLY wherever
float64 decides it.  The helpers of net_cases.py, net_train_cases.py and net_exact_cases.py are used as they are.

The instances.  MULUT_NET_LAUNCH (csrc/mulut_net_dev.h) instantiates the table, pass, stage and stage_sum kernels for MT = 1 (nf <= 32)
or 2 and U = 1..4.  `pairs` lists the (MT, U) of every stage of a model; test_net_grid_cpu.py asserts that the models of tests/ reach
all eight.  GRID_MODELS adds the three that no model had as a unit under a per-value check -- (1, 4), (2, 2), (2, 3) -- with nf 32 a full
single tile, and nf 1, a unit that is all padding.  Each has one stage, so the unit under test is the last stage.

The comparison.  A pass value is round(127 y).  `decided(v64)` is true where the float64 value v64 = 127 y lies further than T from
every half-integer: there a correct kernel, whose 127 y is within T of v64, has no choice, and `exact_where_decided` demands
round(v64) with no exception.  Elsewhere the rule of net_cases.meets stays: off by at most one, and the values that are off at most
BAR of ALL values compared.  A share is taken over all the values of a kind that a model has (see tests/test_net_cpu.py).

T = 8 * MEASURED_Y.  MEASURED_Y is the largest |127 y32 - 127 y64| of the float32 torch path against float64 over every stage of
GRID_MODELS and SEEDED (the seeded models of tests/test_gpu_net.py) on GRID_SHAPES, measured on the CPU: test_net_grid_cpu.py prints it
and asserts it.  With the input bytes of `forward_case` it is 1.49e-4, with the draws the cases were chosen on it was 1.67e-4, both at
nf 64 "eho" on 1 x 1 x 33 x 65; the constant is the larger of the two, rounded up, so T = 1.36e-3.  The factor 8 is the one of
net_train_cases.C, for the same reason: another summation order, MFMA pair chains and a device tanhf over sums of the same length and
type.  The undecided share is about 2 T = 0.27 %; test_net_grid_cpu.py caps it at 1 % of the values of a model.
"""
import copy

import numpy as np
import torch

import net_cases as nc
import net_train_cases as tc
from test_gpu_net import SEEDED      # noqa: F401  (re-exported; a list of dictionaries: importing it needs no GPU)

GRID_MODELS = [dict(nf=32, scale=4, modes="sy", stages=1, seed=11),      # (1, 4), a full single tile
               dict(nf=40, scale=2, modes="dh", stages=1, seed=12),      # (2, 2)
               dict(nf=48, scale=3, modes="so", stages=1, seed=13),      # (2, 3)
               dict(nf=1, scale=2, modes="s", stages=1, seed=14)]        # a unit that is all padding
# one site; a row and a column shorter than every pad; a plane boundary inside a wave tile; one past a 32- and a 128-site tile
GRID_SHAPES = [(1, 3, 1, 1), (1, 1, 1, 9), (1, 1, 9, 1), (2, 3, 5, 7), (1, 1, 33, 65)]
MEASURED_Y = 1.7e-4
T = 8 * MEASURED_Y
MAX_UNDECIDED = 0.01
ALL_PAIRS = {(mt, u) for mt in (1, 2) for u in (1, 2, 3, 4)}

# Stage shapes that only the C ABI can express: a list of (model, the letters taken from it), the units in that order.
# M = MULUT_MAX_MODES = 8 needs a repeated letter; the second needs units of different nf under one padded width.
_WIDE1 = dict(nf=24, scale=2, modes="sdyeho", stages=1)
EIGHT = [(dict(_WIDE1, seed=5), "sdyeho"), (dict(_WIDE1, seed=6), "sd")]
MIXED = [(dict(nf=8, scale=2, modes="s", stages=1, seed=21), "s"), (dict(nf=24, scale=2, modes="y", stages=1, seed=22), "y")]

_cache = {}


def pairs(cfg):
    """(MT, U) of the units of every stage of a model: net_tiles of csrc/mulut_net.h, and u = scale on the last stage only."""
    mt = 1 if cfg["nf"] <= 32 else 2
    return [(mt, cfg["scale"] if s == cfg["stages"] else 1) for s in range(1, cfg["stages"] + 1)]


def nets(cfg, device="cpu"):
    """(the float32 model on the CPU, its float64 copy on `device`) -- shared, read only."""
    key = ("nets", tc.model_id(cfg), cfg["seed"], str(device))
    if key not in _cache:
        net = nc.seeded_model(**cfg)
        _cache[key] = (net, copy.deepcopy(net).double().to(device))
    return _cache[key]


def terms(net, x_u8, modes, stage, dtype):
    """[4 M, N, C, H u, W u] in `dtype`: 127 y of every (mode, rotation) pass, rotated back and NOT rounded, mode outer."""
    with torch.no_grad():
        return torch.stack(tc.stage_terms(net, nc._unit_interval(x_u8, dtype), modes, stage, False))


def input_bytes(cfg, shape):
    rng = np.random.default_rng([cfg["seed"], 77] + list(shape))
    return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))


def rounded(v64):
    return np.rint(np.asarray(v64, np.float64)).astype(np.int64)


def forward_case(cfg, shape, device="cpu"):
    """Per stage (x: the uint8 input on `device`, v64: float64 NumPy [4 M, ...] of `terms`, last).  Stage 1 reads seeded random bytes,
    a later stage the bytes the float64 values of the stage before give."""
    key = ("fwd", tc.model_id(cfg), cfg["seed"], shape, str(device))
    if key not in _cache:
        net64 = nets(cfg, device)[1]
        x, out = input_bytes(cfg, shape).to(device), []
        for s in range(1, cfg["stages"] + 1):
            v64 = terms(net64, x, cfg["modes"], s, torch.float64).cpu().numpy()
            out.append((x, v64, s == cfg["stages"]))
            x = torch.from_numpy(nc.epilogue(rounded(v64), s == cfg["stages"])).to(device)
        _cache[key] = out
    return _cache[key]


def table_values(unit64, interval):
    """float64 [L^4, u u] on the unit's device: 127 y of a MuLUTUnit on the grid 0, q, ..., 256 - q, 255 (each / 255), row = the base-L
    digits a, b, c, d with a slowest (sr/2_transfer_to_lut.py:12-41)."""
    p = next(unit64.parameters())
    v = torch.clamp(torch.arange(0, 257, 1 << interval, device=p.device), max=255).to(p.dtype) / 255.0
    with torch.no_grad():
        return unit64.features(torch.cartesian_prod(v, v, v, v)) * 127


# ------------------------------------------------------------------------------------------------------------------ the comparison
def decided(v64, t=None):
    """True where the float64 value lies further than t (default T) from every half-integer."""
    v = np.asarray(v64, np.float64)
    return np.abs(v - np.floor(v) - 0.5) > (T if t is None else t)


def exact_where_decided(got, v64, what, cap=nc.BAR):
    """got (integers) against v64 (float64, the same shape): equal to round(v64) at every decided position; at the others off by at
    most one, and those that are off at most `cap` of all values.  Returns the number of undecided positions."""
    got, v = np.asarray(got).astype(np.int64).ravel(), np.asarray(v64, np.float64).ravel()
    assert got.shape == v.shape, (what, got.shape, v.shape)
    want, dec = rounded(v), decided(v)
    bad = np.flatnonzero(dec & (got != want))
    d = np.abs(got - want)[~dec]
    worst, off = (int(d.max()), int((d != 0).sum())) if d.size else (0, 0)
    print("%s: %d of %d values undecided; of those %d off, worst %d (cap %.3g of all); %d decided values wrong"
          % (what, d.size, v.size, off, worst, cap, bad.size))
    assert bad.size == 0, (what, "decided values wrong", [(int(i), int(got[i]), float(v[i])) for i in bad[:8]])
    assert worst <= 1 and off <= cap * v.size, (what, worst, off, v.size)
    return int(d.size)


def all_decided(v64):
    """[...] from [4 M, ...]: True where every term of an output is decided."""
    return decided(v64).all(axis=0)


# ---------------------------------------------------------------------------------------------- stages of units from several models
def multi_id(spec):
    return "+".join("nf%d%s" % (cfg["nf"], letters) for cfg, letters in spec)


def multi_modes(spec):
    return "".join(letters for _, letters in spec)


def multi_case(spec, shape, device="cpu"):
    """One stage (the last: u = scale) whose units come from several models, in the order of `spec`: the input bytes, x = bytes / 255, v64
    of its 4 M terms, a kink-free g, and the float64 gradients of sum(smooth sum * g) -- gx64 and, per model, {parameter name: gradient}
    of the units taken from it.  The kinks are taken out over the units of ALL models (net_train_cases.py)."""
    key = ("multi", multi_id(spec), shape, str(device))
    if key not in _cache:
        u = spec[0][0]["scale"]
        assert all(cfg["scale"] == u and cfg["stages"] == 1 for cfg, _ in spec)
        models = [nets(cfg, device) for cfg, _ in spec]
        xb = input_bytes(spec[0][0], shape).to(device)
        v64 = torch.cat([terms(n64, xb, letters, 1, torch.float64) for (_, n64), (_, letters) in zip(models, spec)]).cpu().numpy()
        x = nc._unit_interval(xb, torch.float32)
        N, Cc, H, W = shape
        rng = np.random.default_rng([spec[0][0]["seed"], 78] + list(shape))
        g = torch.from_numpy(rng.standard_normal((N, Cc, H * u, W * u)).astype(np.float32)).to(device)
        mp = None
        for (_, n64), (_, letters) in zip(models, spec):
            m = tc.min_preact(n64, x.double(), letters, 1)
            mp = m if mp is None else torch.minimum(mp, m)
        g, dropped = tc.kink_free(g, mp, u)
        x64 = x.double().requires_grad_(True)
        for _, n64 in models:
            for p in n64.parameters():
                p.grad = None
        total = sum(tc.smooth_sum(n64, x64, letters, 1) for (_, n64), (_, letters) in zip(models, spec))
        (total * g.double()).sum().backward()
        gp64 = []
        for _, n64 in models:
            gp64.append({n: p.grad.detach().clone() for n, p in n64.named_parameters() if p.grad is not None})
            for p in n64.parameters():
                p.grad = None
        _cache[key] = dict(xb=xb, x=x, v64=v64, g=g, dropped=dropped, gx64=x64.grad.detach().clone(), gp64=gp64, u=u)
    return _cache[key]
