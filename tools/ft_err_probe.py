#!/usr/bin/env python3
"""How far are the fine-tune gradients of the HIP path from the CPU oracle on the big batches?  (GPU box)
Prints, per tensor, max |diff|, max |ref| and the largest element-wise relative error among elements above 1 % of max |ref|.

    tools/ft_err_probe.py [--interval 4|5|6]        GPU module against the float32 oracle (interval 4: synthetic tables and the
                                                    batches of tests/test_gpu_finetune.py; 5 / 6: the batches and tables of
                                                    tests/test_gpu_ft_interval.py, the bs-256 one first)
    tools/ft_err_probe.py --interval 5 --orderings  CPU only: the oracle against ITSELF on the bs-256 batch of
                                                    tests/test_gpu_ft_interval.py with the 256 crops in the given order, reversed
                                                    and in one seeded shuffle -- what a different order of the same float32 sums
                                                    is worth; the bars of that test are twice the worst figure printed here
    tools/ft_err_probe.py --modes eho ...           the same two forms for a list with the 4 x 4 patterns e, h, o (any interval):
                                                    mulut_amd.finetune.MuLUTWide against the oracle with the taps of e, h, o added
                                                    to its PATTERNS / PAD at run time, on the seeded tables and batches of
                                                    tests/test_gpu_ft_wide.py (whose bs-256 bars come from --orderings)
"""
import argparse, os, sys, tempfile
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mulut_amd.synth import natural_frames
from oracle import ft_torch


def synthetic_lut(seed, vnum):      # as tests/test_gpu_finetune.py
    rng = np.random.default_rng(seed)
    return rng.integers(-127, 128, size=(17 ** 4, vnum), dtype=np.int8)


def synthetic_lut_iv(interval, stage, mode, vnum):      # as tests/test_gpu_ft_interval.py
    rng = np.random.default_rng(1000 * interval + 17 * stage + ord(mode))
    return rng.integers(-128, 128, size=((2 ** (8 - interval) + 1) ** 4, vnum), dtype=np.int8)


def fixture_tables(interval):
    fx = np.load(os.path.join(ROOT, "tests", "golden", "interval_fixtures.npz"))
    return {"s%d_%s" % (s, m): fx["iv%d/lut/s%d_%s" % (interval, s, m)].reshape(-1, 16 if s == 2 else 1).astype(np.int8)
            for s in (1, 2) for m in "sdy"}


def natural_batch(rng, shape):
    big = natural_frames(1, 1080, 1920, 1, 11)[0, :, :, 0]
    ys, xs = rng.integers(0, 1080 - shape[2], shape[0]), rng.integers(0, 1920 - shape[3], shape[0])
    return np.stack([big[a:a + shape[2], b:b + shape[3]] for a, b in zip(ys, xs)])[:, None].astype(np.float32) / np.float32(255)


def stat(shape, name, g, r):
    d = np.abs(g - r); m = np.abs(r).max()
    sig = np.abs(r) > 0.01 * m
    rel = (d[sig] / np.abs(r[sig])).max() if sig.any() else 0.0
    print("%s %-8s max|diff| %.3e  max|ref| %.3e  ratio %.2e  max rel (|ref| > 1%% of max) %.2e" % (shape, name, d.max(), m, d.max() / m, rel), flush=True)
    return d.max() / m, rel


def oracle_grads(tabs, x, tgt, stages, modes, scale, interval):
    wcpu = {k: torch.from_numpy(v.astype(np.float32) / 127.0).requires_grad_(True) for k, v in tabs.items()}
    xc = torch.from_numpy(x).requires_grad_(True)
    yc = ft_torch.forward(wcpu, xc, stages, modes, scale, interval)
    torch.nn.functional.mse_loss(yc, torch.from_numpy(tgt)).backward()
    return xc.grad.numpy(), {k: w.grad.numpy() for k, w in wcpu.items()}


WIDE_PATTERNS = {"e": ((0, 0), (0, 3), (3, 0), (3, 3)), "h": ((0, 0), (2, 2), (2, 3), (3, 2)), "o": ((0, 0), (2, 2), (1, 3), (3, 1))}


def extend_oracle():
    """the taps of e, h, o (common/network.py:173-215), edge pad 3, for this process (tests/ft_wide_cases.py does it per test)"""
    ft_torch.PATTERNS = dict(ft_torch.PATTERNS, **WIDE_PATTERNS)
    ft_torch.PAD = dict(ft_torch.PAD, e=3, h=3, o=3)


def case(interval, shape, kind, modes="sdy"):
    """(tables, x, target) of one batch: the test files' own draws."""
    stages, scale = 2, 4
    if modes != "sdy":      # tests/test_gpu_ft_wide.py: seeded tables at every interval
        rng = np.random.default_rng(stages * 100 + scale * 10 + len(modes) + interval)
        tabs = {"s%d_%s" % (s + 1, m): synthetic_lut_iv(interval, s + 1, m, scale * scale if s + 1 == stages else 1) for s in range(stages) for m in modes}
        x = natural_batch(np.random.default_rng(1), shape) if kind == "smooth" else rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)
    elif interval == 4:
        rng = np.random.default_rng(241)
        tabs = {"s%d_%s" % (s + 1, m): synthetic_lut(3 * s + ord(m), scale * scale if s + 1 == stages else 1) for s in range(stages) for m in modes}
        x = natural_batch(rng, shape) if kind == "smooth" else rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)
    else:
        rng = np.random.default_rng(stages * 100 + scale * 10 + len(modes) + interval)
        if kind == "smooth":
            tabs, x = fixture_tables(interval), natural_batch(np.random.default_rng(1), shape)
        else:
            tabs = {"s%d_%s" % (s + 1, m): synthetic_lut_iv(interval, s + 1, m, scale * scale if s + 1 == stages else 1) for s in range(stages) for m in modes}
            x = rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)
    tgt = rng.random((shape[0], shape[1], shape[2] * scale, shape[3] * scale), dtype=np.float32)
    return tabs, x, tgt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--interval", type=int, default=4, choices=(4, 5, 6))
    ap.add_argument("--orderings", action="store_true")
    ap.add_argument("--modes", default="sdy", help="sdy: the batches of the s, d, y tests; any other list over sdyeho: MuLUTWide")
    opt = ap.parse_args()
    stages, modes, scale = 2, opt.modes, 4
    if any(m in "eho" for m in modes):
        extend_oracle()
    if opt.orderings:
        shape = (256, 1, 48, 48)
        tabs, x, tgt = case(opt.interval, shape, "smooth", modes)
        perms = [np.arange(256), np.arange(256)[::-1].copy(), np.random.default_rng(7).permutation(256)]
        res = []
        for p in perms:
            gx, gw = oracle_grads(tabs, x[p], tgt[p], stages, modes, scale, opt.interval)
            inv = np.argsort(p)
            res.append((gx[inv], gw))
        worst = [0.0, 0.0]
        for a, b, name in ((0, 1, "given/reversed"), (0, 2, "given/shuffled"), (1, 2, "reversed/shuffled")):
            print(name)
            stat(shape, "gx", res[a][0], res[b][0])
            for k in res[a][1]:
                n, e = stat(shape, k, res[a][1][k], res[b][1][k])
                worst = [max(worst[0], n), max(worst[1], e)]
        print("interval %d worst over the table gradients: norm-wise %.3e element-wise %.3e" % (opt.interval, worst[0], worst[1]))
        return
    from mulut_amd.finetune import MuLUT, MuLUTInterval, MuLUTWide
    cls = MuLUTWide if modes != "sdy" else MuLUT if opt.interval == 4 else MuLUTInterval
    for shape, kind in (((256, 1, 48, 48), "smooth"), ((16, 1, 48, 48), "u8"), ((256, 1, 48, 48), "u8")):
        tabs, x, tgt = case(opt.interval, shape, kind, modes)
        tmp = tempfile.mkdtemp()
        for k, t in tabs.items():
            np.save(os.path.join(tmp, "LUT_x%d_%dbit_int8_%s.npy" % (scale, opt.interval, k)), t)
        gxc, gwc = oracle_grads(tabs, x, tgt, stages, modes, scale, opt.interval)
        net = cls(tmp, stages, modes, upscale=scale, interval=opt.interval).cuda()
        xg = torch.from_numpy(x).cuda().requires_grad_(True)
        yg = net(xg)
        torch.nn.functional.mse_loss(yg, torch.from_numpy(tgt).cuda()).backward()
        worst = [0.0, 0.0]
        stat(shape, "gx", xg.grad.cpu().numpy(), gxc)
        for k, r in gwc.items():
            n, e = stat(shape, k, getattr(net, "weight_" + k).grad.cpu().numpy(), r)
            worst = [max(worst[0], n), max(worst[1], e)]
        print("interval %d %s %s worst over the table gradients: norm-wise %.3e element-wise %.3e" % (opt.interval, shape, kind, worst[0], worst[1]), flush=True)


if __name__ == "__main__":
    main()
