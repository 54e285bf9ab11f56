"""What tests/test_net_cpu.py and tests/test_gpu_net.py share: the fixture of gen_golden_net.py read back as one dictionary, the two
models it was made with, a torch restatement of `mulut_predict(..., 'valid')` (sr/1_train_model.py:26-45,93-101) over
`network.SRNets`, the stage epilogue in integers, and the bar.

The bar (tests/test_transfer_cpu.py): a value is round(127 * tanh(...)); a different summation order can move one that sits within
float rounding of a .5 boundary by one step.  So no value is off by more than 1 and at most 1e-4 of the values are off at all.  A byte
of a stage that was fed the reference's own input bytes can differ only where one of its 4 M pass values did: share <= 4 M * 1e-4,
and for M >= 2 no byte off by more than 1 (one pass value off by one moves pred / M or pred / (4 M) by at most 1/2).  The cascade on
its own bytes: share <= stages * 4 M * 1e-4 (and no bound on a single byte: see meets).
"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN

from mulut_amd import network

BAR = 1e-4
SET5 = ("baby", "bird", "butterfly", "head", "woman")
MODELS = {"shipped": dict(nf=64, scale=4, modes="sdy", stages=2), "tiny": dict(nf=8, scale=2, modes="sdy", stages=1)}
_cache = {}


def fixture():
    """net_fixtures.npz and its shards net_fixtures_pass<k>.npz as one {key: array}."""
    if "fx" not in _cache:
        fx = {}
        for path in sorted(glob.glob(os.path.join(GOLDEN, "net_fixtures*.npz"))):
            with np.load(path) as f:
                fx.update({k: f[k] for k in f.files})
        _cache["fx"] = fx
    return _cache["fx"]


def cases(model):
    fx = fixture()
    return sorted({k.split("/")[1] for k in fx if k.startswith(model + "/")})


def model(name):
    """The `SRNets` a fixture model was made from: the shipped checkpoint, or the seeded tiny one from transfer_fixtures.npz."""
    if name not in _cache:
        cfg = MODELS[name]
        net = network.SRNets(nf=cfg["nf"], scale=cfg["scale"], modes=list(cfg["modes"]), stages=cfg["stages"])
        if name == "shipped":
            sd = network.load_checkpoint(os.path.join(GOLDEN, "Model_200000.pth")).state_dict()
        else:
            with np.load(os.path.join(GOLDEN, "transfer_fixtures.npz")) as f:
                sd = {k[len("tinyw/"):]: torch.from_numpy(f[k]) for k in f.files if k.startswith("tinyw/")}
        net.load_state_dict(sd, strict=True)
        _cache[name] = net.eval()
    return _cache[name]


def seeded_model(nf, scale, modes, stages, seed):
    torch.manual_seed(seed)
    net = network.SRNets(nf=nf, scale=scale, modes=list(modes), stages=stages).eval()
    with torch.no_grad():
        for p in net.parameters():      # MSRA weights with zero biases leave tanh near 0: give every layer a bias
            if p.dim() == 1:
                p.uniform_(-0.2, 0.2)
    return net


# byte / 255 as the host divides it (float32, correctly rounded): a device division may be a product with a rounded reciprocal
_BYTE = torch.arange(256, dtype=torch.float32) / 255.0


def _unit_interval(x_u8, dtype):
    return _BYTE.to(device=x_u8.device, dtype=dtype)[x_u8.long()] if dtype == torch.float32 else x_u8.to(dtype) / 255.0


def predict_valid(net, x_u8, modes, stages, dtype=torch.float32):
    """`mulut_predict` in the 'valid' phase, restated, on uint8 [N, C, H, W] (any device): per stage the 4 M rounded passes
    (int8 [4 M, N, C, H u, W u], mode outer and rotation inner) and the stage's bytes; the last stage's bytes are the result."""
    M = len(modes)
    out = []
    x = x_u8
    with torch.no_grad():
        for s in range(1, stages + 1):
            xf = _unit_interval(x, dtype)
            passes = []
            for mode in modes:
                pad = network.TAPS[mode.upper()][0] - 1
                for r in range(4):
                    y = net(F.pad(torch.rot90(xf, r, [2, 3]), (0, pad, 0, pad), mode="replicate"), stage=s, mode=mode)
                    passes.append(torch.round(torch.rot90(y, (4 - r) % 4, [2, 3]) * 127))
            pred = torch.stack(passes).sum(0)
            if s == stages:
                x = torch.clamp(torch.round(pred / M), 0, 255).to(torch.uint8)
            else:
                x = torch.round(torch.clamp(pred / (4 * M) + 127, 0, 255)).to(torch.uint8)
            out.append((torch.stack(passes).to(torch.int8), x))
    return out


def epilogue(passes_i8, is_last):
    """The stage epilogue in integers on int8 [4 M, ...] -> uint8: clip(rhe(pred / (4 M) + 127)) or, last, clip(rhe(pred / M))."""
    p = np.asarray(passes_i8).astype(np.int64)
    M = p.shape[0] // 4
    pred = p.sum(0)
    D = M if is_last else 4 * M
    n = pred + (0 if is_last else 127 * D)
    q, rem = np.divmod(n, D)      # floor division: rem in [0, D)
    q = q + ((2 * rem > D) | ((2 * rem == D) & (q % 2 == 1)))
    return np.clip(q, 0, 255).astype(np.uint8)


def off(got, want):
    """(largest difference, share of values that differ) of two integer arrays of one shape."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), float((d != 0).mean())


def meets(got, want, cap=BAR, what="", by_one=True):
    """by_one=False: the cascade on its own bytes -- a first-stage byte off by one is another INPUT of the next stage, whose output may
    then differ by any amount, so only the share is bounded there."""
    worst, share = off(got, want)
    print("%s: worst %d, share off %.3g of %d (cap %.3g)" % (what, worst, share, np.asarray(want).size, cap))
    assert (worst <= 1 or not by_one) and share <= cap, (what, worst, share, cap)
