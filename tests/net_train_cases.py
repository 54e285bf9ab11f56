"""What tests/test_net_train_cpu.py and tests/test_gpu_net_train.py share: the fixture of gen_golden_net_train.py, its two models, a
torch restatement of `mulut_predict(..., 'train')` (sr/1_train_model.py:26-55) over `network.SRNets` that can be forced to given
per-stage sums, the op-level cases (inputs, a kink-free g, the float64 reference), and the gradient bar.

The gradient bar.  The op's gradient is the Jacobian of the smooth sum of 127 * net at x (round is the identity in the backward).  In
float32 a pre-activation within float rounding of 0 may take the other ReLU branch than in float64, and with a zero-mean g one such
site is visible in a sum over 10^4..10^5 sites, so a case takes the kinks OUT rather than loosening the bar: `min_preact` is, in
float64, each pixel's smallest |pre-activation| over layers 1-5 of its 4 M sites, and `kink_free` zeroes g on the u x u block of
every pixel below TAU -- there delta_6 = 0 and the site contributes nothing whichever branch it took.  No case may drop more than
MAX_DROP of its pixels.  Per tensor then  max |got - ref64| <= C * max |ref64|,  C = 8 x the largest such distance of the float32
torch path over the committed case list (the factor 8: another summation order, MFMA pair chains and split partials over sums of the
same length and type).  test_net_train_cpu.py measures that distance, prints it and asserts it is <= C / 8.
"""
import copy
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN

from mulut_amd import network
import net_cases as nc

TAU = 1e-5
MAX_DROP = 0.10
# The float32 torch path against float64, measured on the CPU over OP_MODELS x OP_SHAPES x stages (test_net_train_cpu.py prints it):
# parameters 9.03e-6 (the conv6 bias of s1_h of the nf 24 model on 1 x 1 x 33 x 65: a sum of 8,580 zero-mean terms that cancel; the
# next largest is 2.5e-6), gx 9.87e-7; on the fixture batches 3.1e-7.  The two constants below are those, rounded up.
MEASURED_P, MEASURED_X = 9.1e-6, 1.0e-6
C = 8 * MEASURED_P
LOSS_RTOL = 1e-6

MODELS = {"tiny": dict(nf=8, scale=2, modes="sdy", stages=1), "sd2": dict(nf=8, scale=2, modes="sd", stages=2)}
# the seeded models of tests/test_gpu_net.py: one and two feature tiles with padding, every u, pad-3 patterns
OP_MODELS = [dict(nf=8, scale=3, modes="sd", stages=2, seed=1), dict(nf=64, scale=4, modes="eho", stages=1, seed=2),
             dict(nf=24, scale=2, modes="sdyeho", stages=2, seed=5), dict(nf=33, scale=1, modes="y", stages=2, seed=3)]
# 1 site; rows / columns shorter than every pad; plane boundaries inside a tile; one past a 32- and a 128-site tile each way
OP_SHAPES = [(1, 3, 1, 1), (1, 1, 1, 9), (1, 1, 9, 1), (2, 3, 5, 7), (1, 1, 33, 65), (2, 3, 65, 33)]
_cache = {}


def model_id(cfg):
    return "nf%d_x%d_%s_%d" % (cfg["nf"], cfg["scale"], cfg["modes"], cfg["stages"])


def fixture():
    if "fx" not in _cache:
        with np.load(os.path.join(GOLDEN, "net_train_fixtures.npz")) as f:
            _cache["fx"] = {k: f[k] for k in f.files}
    return _cache["fx"]


def cases(name):
    return sorted({k.split("/")[1] for k in fixture() if k.startswith(name + "/")})


def model(name):
    """A fixture model, float32 on the CPU (a fresh copy: callers move and train it)."""
    cfg = MODELS[name]
    net = network.SRNets(nf=cfg["nf"], scale=cfg["scale"], modes=list(cfg["modes"]), stages=cfg["stages"])
    if name == "tiny":
        with np.load(os.path.join(GOLDEN, "transfer_fixtures.npz")) as f:
            sd = {k[len("tinyw/"):]: torch.from_numpy(f[k]) for k in f.files if k.startswith("tinyw/")}
    else:
        sd = {k[len(name + "w/"):]: torch.from_numpy(v) for k, v in fixture().items() if k.startswith(name + "w/")}
    net.load_state_dict(sd, strict=True)
    return net


def round_func(x):
    out = x.clone()
    out.data = torch.round(x).data
    return out


def stage_terms(net, x, modes, stage, rounded):
    """The 4 M terms of a stage's pred, rotated back (mode outer, rotation inner): round_func'ed as the reference has them, or smooth."""
    out = []
    for mode in modes:
        pad = network.TAPS[mode.upper()][0] - 1
        for r in range(4):
            y = torch.rot90(net(F.pad(torch.rot90(x, r, [2, 3]), (0, pad, 0, pad), mode="replicate"), stage=stage, mode=mode), (4 - r) % 4, [2, 3]) * 127
            out.append(round_func(y) if rounded else y)
    return out


def smooth_sum(net, x, modes, stage):
    return torch.stack(stage_terms(net, x, modes, stage, False)).sum(0)


def predict_train(net, x, modes, stages, forced=None, phase="train"):
    """`mulut_predict` restated.  Returns (result, [pred of every stage]).  forced: per stage a tensor that replaces pred's VALUE
    (`pred.data = forced`, the trick round_func plays) while the graph stays pred's."""
    M, sums = len(modes), []
    for s in range(1, stages + 1):
        pred = 0
        for t in stage_terms(net, x, modes, s, True):
            pred = pred + t
        if forced is not None:
            pred = pred.clone()
            pred.data = forced[s - 1].to(pred.dtype).data
        sums.append(pred)
        if s == stages:
            x = round_func(pred / M + 0)
            if phase == "train":
                x = x / 255.0
        else:
            x = round_func(torch.clamp(pred / (M * 4) + 127, 0, 255)) / 255.0
    return x, sums


def min_preact(net, x, modes, stage):
    """[N, C, H, W]: per pixel the smallest |pre-activation| over layers 1-5 of the 4 M sites anchored at it (in the dtype of net, x)."""
    out = None
    with torch.no_grad():
        for mode in modes:
            srn = getattr(net, "s{}_{}".format(stage, mode))
            P = srn.P
            for r in range(4):
                xp = F.pad(torch.rot90(x, r, [2, 3]), (0, P, 0, P), mode="replicate")
                B, Cc, H, W = xp.shape
                h, w = H - P, W - P
                t = torch.stack([xp[:, :, i:i + h, j:j + w] for (i, j) in network.TAPS[mode.upper()][1]], dim=-1).reshape(-1, 4)
                unit = srn.model
                wm, b = unit.conv1.matrix()
                pre = F.linear(t, wm, b)
                m = pre.abs().min(1).values
                a = F.relu(pre)
                for layer in (unit.conv2, unit.conv3, unit.conv4, unit.conv5):
                    wm, b = layer.conv1.matrix()
                    pre = F.linear(a, wm, b)
                    m = torch.minimum(m, pre.abs().min(1).values)
                    a = torch.cat([a, F.relu(pre)], dim=1)
                m = torch.rot90(m.reshape(B, Cc, h, w), (4 - r) % 4, [2, 3])
                out = m if out is None else torch.minimum(out, m)
    return out


def kink_free(g, mp, u, tau=TAU):
    """g with the u x u block of every pixel whose min_preact is below tau set to 0, and the share of pixels dropped."""
    drop = mp < tau
    keep = (~drop).to(g.dtype).repeat_interleave(u, 2).repeat_interleave(u, 3)
    return g * keep, float(drop.double().mean())


def op_reference(net, x, g, modes, stage, want_gx=True):
    """(gx or None, {parameter name: gradient}) of sum(smooth_sum * g) in the dtype and on the device of net, x, g."""
    x = x.detach().clone().requires_grad_(want_gx)
    for p in net.parameters():
        p.grad = None
    (smooth_sum(net, x, modes, stage) * g).sum().backward()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    for p in net.parameters():
        p.grad = None
    return (x.grad.detach().clone() if want_gx else None), grads


def op_case(cfg, shape, stage, device="cpu"):
    """One op-level case: x (random bytes / 255, float32), a kink-free g, the float64 model and reference, the share dropped."""
    key = (model_id(cfg), shape, stage, str(device))
    if key not in _cache:
        net = nc.seeded_model(**cfg)
        net64 = copy.deepcopy(net).double().to(device)
        u = cfg["scale"] if stage == cfg["stages"] else 1
        N, Cc, H, W = shape
        for draw in range(8):      # on a shape of 9 pixels one dropped pixel is 11 %: such a draw of x is passed over (the same on every machine)
            rng = np.random.default_rng([cfg["seed"], stage, draw] + list(shape))
            x = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8).astype(np.float32) / 255.0).to(device)
            g = torch.from_numpy(rng.standard_normal((N, Cc, H * u, W * u)).astype(np.float32)).to(device)
            g, dropped = kink_free(g, min_preact(net64, x.double(), cfg["modes"], stage), u)
            if dropped <= MAX_DROP:
                break
        gx64, gp64 = op_reference(net64, x.double(), g.double(), cfg["modes"], stage)
        _cache[key] = dict(net=net, x=x, g=g, gx64=gx64, gp64=gp64, dropped=dropped, u=u)
    return _cache[key]


def distance(got, ref):
    """max |got - ref| / max |ref| (0 / 0 = 0)."""
    ref = ref.double()
    top = float(ref.abs().max())
    d = float((got.double().to(ref.device) - ref).abs().max())
    return 0.0 if d == 0.0 else d / top if top > 0 else float("inf")


def meets(got, ref, what, c=C):
    d = distance(got, ref)
    print("%s: %.3g of max |ref| (bar %.3g)" % (what, d, c))
    assert d <= c, (what, d, c)
    return d
