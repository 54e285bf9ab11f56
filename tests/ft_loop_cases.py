"""The fine-tune LOOP held to the reference one step at a time (test infrastructure, shared by test_ft_loop_cpu.py and
test_gpu_ft_loop.py): a reference stepper for mulut_amd/finetune_lut.py::FinetuneRun, the twin of sr/3_finetune_lut.py:68-172.

Why one step at a time: a failure then names its step and its part (forward, loss, gradient, optimiser, schedule), each held to a bar
of its own -- bytes for the forward, float32 ulps for the optimiser -- and the device's atomics, which sum a gradient in another
order on every run, never reach a later step's reference.  The stepper therefore starts every step from the state the device holds
before it, and its optimiser is fed the gradient the device produced.  (The float32 and the plain float64 oracle do part by full
Adam steps, but because the latter's x * 255 is not integer-valued, not because Adam amplifies rounding noise:
test_ft_loop_cpu.py::test_float32_and_float64_oracles_part_by_full_adam_steps_and_why.)

Nothing is imported from the code under test.  The pieces:
  forward and gradients   oracle/ft_torch.forward (under ft_wide_cases.wide_oracle() for lists with e, h, o).  In float64 with
                          quant_f32: the input's * 255 and the quantisation clamp(round(w * 127), -127, 127) are done in float32,
                          where the reference decides its ties; everything after them runs in float64.
  adam_step               sr/3_finetune_lut.py:86 in float64 on an explicit state (test_ft_loop_cpu.py pins it to torch.optim.Adam)
  lf / lr_at              the two cosine forms of :89-95; step i runs at lr0 * lf(i - 1)
  write_pairs / batches   three synthetic training pairs and CropProvider's batches restated (random.Random(seed) in its
                          order, the crop of sr/data.py:101-119 through crop_cases.apply_draws); the GPU file asserts that a real
                          CropProvider gives the same arrays
  start_tables            the tables a case starts from, a stated handful of entries forced to +-127
"""
import collections
import contextlib
import math
import os
import random

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

import abi_sequences as A
from conftest import GOLDEN
from crop_cases import apply_draws
from ft_wide_cases import wide_oracle
from oracle import ft_torch

SEED = 5
# The loss bar: |F.mse_loss in float32 - in float64| / the float64 loss on the CPU, on the oracle's own output, largest over all cases
# and steps of the float32 free run (test_ft_loop_cpu.py measures it: 1.76e-7, case A step 1, and holds this constant to within a factor
# of two of what it measures).  The device reduces in another order: test_gpu_ft_loop.py allows 4 x this.
LOSS_F32_REL = 1.8e-7
DISPLAY_STEP = 4      # with K = 6 one display point and a tail of two steps behind it; with K = 8 two display points

Case = collections.namedtuple("Case", "name interval stages modes scale batch crop lr0 lr1 wd K")

# The smallest shapes at which every table, both clamps and both halo widths are touched.  lr0 = 1e-2 moves w * 127 by up to 1.27 per
# step: quantised entries change on every step and entries that start at +-127 leave the quantiser's clamp on the first.  D keeps the
# reference's 1e-3 (0.127 per step: the first change falls on the fourth or fifth step) and runs 8 steps.
CASES = collections.OrderedDict((c.name, c) for c in (
    Case("A", 4, 2, "sdy", 4, 8, 16, 1e-2, 1e-4, 0.0, 6),
    Case("B", 4, 1, "s", 2, 4, 12, 1e-2, -1.0, 1e-2, 6),
    Case("C", 5, 2, "sdy", 4, 8, 16, 1e-2, 1e-3, 0.0, 6),
    Case("D", 6, 3, "sd", 3, 4, 12, 1e-3, 1e-4, 1e-3, 8),
    Case("E", 4, 2, "se", 2, 4, 12, 1e-2, 1e-4, 0.0, 6),
    Case("F", 6, 1, "sdyeho", 4, 4, 12, 1e-2, -1.0, 0.0, 6),
))


def keys(case):
    return ["s%d_%s" % (s + 1, m) for s in range(case.stages) for m in case.modes]


def oracle_ctx(case):
    return wide_oracle() if any(m in "eho" for m in case.modes) else contextlib.nullcontext()


# ------------------------------------------------------------------------------------------------------------------- schedule
def lf(case, x):
    """sr/3_finetune_lut.py:89-95 with totalIter = case.K"""
    c = ((1 + math.cos(x * math.pi / case.K)) / 2) ** 1.0
    if case.lr1 < 0:
        return c * 0.8 + 0.2
    lr_b = case.lr1 / case.lr0
    return c * (1 - lr_b) + lr_b


def lr_at(case, i):
    """The learning rate of step i = 1..K: LambdaLR sets lr0 * lf(0) when it is built and lr0 * lf(n) in its n-th step(), which the
    loop calls AFTER the optimiser's n-th (:135-136)."""
    return case.lr0 * lf(case, i - 1)


# ----------------------------------------------------------------------------------------------------------------------- Adam
def adam_step(p, g, exp_avg, exp_avg_sq, step, lr, wd, beta1=0.9, beta2=0.999, eps=1e-8):
    """optim.Adam(betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, amsgrad=False) (sr/3_finetune_lut.py:86) on float64 arrays:
    (p, exp_avg, exp_avg_sq, step) after one step.  L2 weight decay goes into the gradient."""
    p, g, exp_avg, exp_avg_sq = (np.asarray(a, np.float64) for a in (p, g, exp_avg, exp_avg_sq))
    step = step + 1
    if wd != 0:
        g = g + wd * p
    exp_avg = exp_avg + (g - exp_avg) * (1 - beta1)
    exp_avg_sq = exp_avg_sq * beta2 + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = np.sqrt(exp_avg_sq) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (exp_avg / denom), exp_avg, exp_avg_sq, step


def torch_adam_step(p, g, exp_avg, exp_avg_sq, step, lr, wd, dtype):
    """The same step by torch.optim.Adam(foreach=False, fused=False) on CPU tensors of `dtype`, from the same explicit state."""
    t = torch.nn.Parameter(torch.tensor(np.asarray(p), dtype=dtype))
    opt = torch.optim.Adam([t], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, amsgrad=False, foreach=False, fused=False)
    opt.state[t] = {"step": torch.tensor(float(step)), "exp_avg": torch.tensor(np.asarray(exp_avg), dtype=dtype),
                    "exp_avg_sq": torch.tensor(np.asarray(exp_avg_sq), dtype=dtype)}
    t.grad = torch.tensor(np.asarray(g), dtype=dtype)
    opt.step()
    st = opt.state[t]
    return t.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), int(st["step"].item())


def ulps32(got, want64):
    """|got - want| in units of the float32 ulp of each element of want (float64 result rounded to float32)"""
    w32 = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want64, np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------ data
LR_H, LR_W = 24, 20


def pair_images(scale):
    """[(lr, hr)] as CropProvider holds them (H x W x C uint8): photograph-like HR (mulut_amd.synth.natural_frames), LR its box
    average; the second pair is grey."""
    from mulut_amd.synth import natural_frames
    out = []
    for n, ch in enumerate((3, 1, 3)):
        hr = natural_frames(1, LR_H * scale, LR_W * scale, ch, seed=40 + n)[0]
        lr = hr.reshape(LR_H, scale, LR_W, scale, ch).mean(axis=(1, 3)).round().astype(np.uint8)
        out.append((lr, hr))
    return out


def write_pairs(root, scale):
    """{root}/HR/im<n>.png with {root}/LR/X{scale}/im<n>x{scale}.png (the DIV2K layout); returns root"""
    root = str(root)
    os.makedirs(os.path.join(root, "HR"))
    os.makedirs(os.path.join(root, "LR", "X%d" % scale))
    for n, (lr, hr) in enumerate(pair_images(scale)):
        sq = (lambda a: a[:, :, 0]) if hr.shape[2] == 1 else (lambda a: a)
        Image.fromarray(sq(hr)).save(os.path.join(root, "HR", "im%d.png" % n))
        Image.fromarray(sq(lr)).save(os.path.join(root, "LR", "X%d" % scale, "im%dx%d.png" % (n, scale)))
    return root


def batches(case, seed=SEED):
    """The K batches (im [B,1,sz,sz], lb [B,1,sz*s,sz*s], float32 in 0..1) CropProvider(..., seed) cuts from write_pairs' set: its draws
    (pair, i, j, c, flip lr, flip ud, k per sample, in that order, from random.Random(seed)) and the reference's crop."""
    pairs, rng, sz = pair_images(case.scale), random.Random(seed), case.crop
    out = []
    for _ in range(case.K):
        rows = []
        for _ in range(case.batch):
            n = rng.choice(range(len(pairs)))
            h, w, ch = pairs[n][0].shape
            i, j = rng.randint(0, h - sz), rng.randint(0, w - sz)
            c = rng.randrange(ch)
            lr = rng.uniform(0, 1) < 0.5
            ud = rng.uniform(0, 1) < 0.5
            rows.append((n, i, j, c, lr + 2 * ud, rng.choice([0, 1, 2, 3])))
        out.append(apply_draws(pairs, rows, sz, case.scale))
    return out


# ---------------------------------------------------------------------------------------------------------------------- tables
def forced_rows(case):
    """The rows of a start table whose element 0 is forced: the grid's diagonal (all four keys the same MSB k), which flat image
    regions sample whatever the pattern -- +127 for even k, -127 for odd k.  L entries per table."""
    L = 2 ** (8 - case.interval) + 1
    return [(k * (L ** 3 + L ** 2 + L + 1), 127 if k % 2 == 0 else -127) for k in range(L)]


def start_tables(case):
    """{key: int8 [L^4, u*u]}: case A the shipped tables perturbed as test_finetune_driver_reduces_loss_and_writes_luts does, the
    others abi_sequences.make_table(smooth=True) (-128 included: beyond the quantiser's clamp from the start); then forced_rows."""
    out = {}
    for s in range(case.stages):
        vnum = case.scale ** 2 if s + 1 == case.stages else 1
        for m in case.modes:
            key = "s%d_%s" % (s + 1, m)
            if case.name == "A":
                t = np.load(os.path.join(GOLDEN, "luts", "LUT_ft_x4_4bit_int8_%s.npy" % key)).reshape(-1, vnum)
                rng = np.random.default_rng((s + 1) * 7 + ord(m))
                t = np.clip(t.astype(np.int32) + rng.integers(-12, 13, t.shape), -127, 127).astype(np.int8)
            else:
                t = A.make_table(np.random.default_rng(100 * ord(case.name) + 10 * s + ord(m)), case.interval, vnum, True)
            for row, v in forced_rows(case):
                t[row, 0] = v
            out[key] = t
    return out


def write_tables(case, folder):
    os.makedirs(str(folder), exist_ok=True)
    for key, t in start_tables(case).items():
        np.save(os.path.join(str(folder), "LUT_x%d_%dbit_int8_%s.npy" % (case.scale, case.interval, key)), t)
    return str(folder)


def start_weights(case):
    """float32 int8 / 127, as the module loads them (sr/model.py:49-57)"""
    return {k: t.astype(np.float32) / 127.0 for k, t in start_tables(case).items()}


# ---------------------------------------------------------------------------------------------------------------------- oracle
class Step(object):
    pass


def oracle_step(case, weights, im, lb, dtype=torch.float64):
    """Forward, MSE and gradients of one step from `weights` ({key: float32 array}) on the batch (im, lb: float32 arrays).
    float64: quant_f32 (see the module docstring); float32: the reference as it runs.  Returns a Step with
      out      [B,1,H,W] float64, the output * 255 -- integer-valued (asserted)
      loss     float, F.mse_loss in `dtype`
      out_t    the output tensor (dtype), for a loss in another precision
      grads    {key: array of dtype}
      beyond   {key: bool array}: |round(w * 127)| > 127 in float32 -- the quantiser's clamp stops the gradient there
      pred     the last stage's un-clamped pred / avg (float64 array): the final clamp passes gradient where it lies in [0, 255]"""
    f64 = dtype == torch.float64
    tw = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in weights.items()}
    x, y = torch.from_numpy(im).to(dtype), torch.from_numpy(lb).to(dtype)
    preds = []
    with oracle_ctx(case):
        out = ft_torch.forward(tw, x, case.stages, case.modes, case.scale, case.interval, quant_f32=f64, preds=preds)
        loss = F.mse_loss(out, y)
        loss.backward()
    r = Step()
    o255 = out.detach().to(torch.float64).numpy() * 255.0
    r.out = np.rint(o255)
    assert np.abs(o255 - r.out).max() < 1e-4 and r.out.min() >= 0 and r.out.max() <= 255
    r.loss, r.out_t = float(loss.item()), out.detach()
    r.grads = {k: t.grad.numpy() for k, t in tw.items()}
    r.beyond = {k: np.abs(np.round(v.astype(np.float32) * np.float32(127))) > 127 for k, v in weights.items()}
    r.pred = preds[-1].to(torch.float64).numpy() / len(case.modes)
    return r


def quantised(weights):
    """{key: clamp(round(w * 127), -127, 127) in float32}"""
    return {k: np.clip(np.round(v.astype(np.float32) * np.float32(127)), -127, 127) for k, v in weights.items()}
