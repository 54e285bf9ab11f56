#!/usr/bin/env python3
"""What the bit-reproducible backward costs: the fine-tune step (forward + backward + the project's Adam) of 2-stage sdy x4 at
interval 4 on the shipped tables, in ONE process, the default step (float-atomic backward kernels) and the deterministic step
(mulut_ft_exact_stage_backward: 64-bit fixed-point sums) alternating round-robin, at batch 32 and batch 256 of 48 x 48 crops, on
natural-like crops and on uniform noise.  Every leg is warmed up first, then timed for at least --seconds of device-synchronised
steps; medians and min-max per leg, and the ratio deterministic / default per batch and content.  The kernels of the deterministic
step alone -- fx_accumulate, the hot one, and the clear, maximum and finish launches around it -- come from torch.profiler, beside
the default step's backward kernels.
    python tools/ft_exact_bench.py --out profiles/ft_exact_bench.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mulut_amd import _native  # noqa: E402
from mulut_amd.finetune import Adam, MuLUT  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402


def module(deterministic):
    with tempfile.TemporaryDirectory() as td:
        for s in (1, 2):
            for m in "sdy":
                t = np.load(os.path.join(ROOT, "tests", "golden", "luts", "LUT_ft_x4_4bit_int8_s%d_%s.npy" % (s, m)))
                np.save(os.path.join(td, "LUT_x4_4bit_int8_s%d_%s.npy" % (s, m)), t)
        return MuLUT(td, 2, "sdy", upscale=4, interval=4, deterministic=deterministic).cuda()


class Leg:
    def __init__(self, deterministic, x, y):
        self.net, self.x, self.y = module(deterministic), x, y
        self.opt = Adam(self.net.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)

    def step(self):
        self.opt.zero_grad()
        loss = torch.nn.functional.mse_loss(self.net(self.x), self.y)
        loss.backward()
        self.opt.step()
        return loss


def timed(leg):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    leg.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_times(leg, iters=5):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(iters):
            leg.step()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        if t is None:
            t = getattr(e, "cuda_time_total", 0)
        if t > 0 and e.device_type != torch.autograd.DeviceType.CPU:
            out[e.key[:90]] = round(t / iters / 1e3, 4)
    return dict(sorted(out.items(), key=lambda kv: -kv[1])[:12])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crop", type=int, default=48)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per leg, at least")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    big = natural_frames(1, 1080, 1920, 1, 0)[0, :, :, 0]
    rng = np.random.default_rng(0)
    res = {"metric": "LUT fine-tune step (fwd+bwd+Adam), 2-stage sdy x4, interval 4, ms per step: default against deterministic", "crop": a.crop,
           "source_hash": _native.source_hash(), "device": torch.cuda.get_device_name(0)}
    legs = {}
    for bs in (32, 256):
        ys, xs = rng.integers(0, 1080 - a.crop, bs), rng.integers(0, 1920 - a.crop, bs)
        data = {"natural": torch.from_numpy(np.stack([big[p:p + a.crop, q:q + a.crop] for p, q in zip(ys, xs)])[:, None].astype(np.float32) / 255.0).cuda(),
                "noise": torch.randint(0, 256, (bs, 1, a.crop, a.crop), device="cuda", generator=g).float() / 255.0}
        y = torch.rand((bs, 1, a.crop * 4, a.crop * 4), device="cuda", generator=g)
        for kind in ("natural", "noise"):
            for det in (False, True):
                legs["%s_bs%d_%s" % ("deterministic" if det else "default", bs, kind)] = Leg(det, data[kind], y)
    for leg in legs.values():      # warm-up of every leg first
        for _ in range(3):
            leg.step()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    while any(sum(v) < a.seconds * 1e3 or len(v) < 5 for v in times.values()):      # round-robin: the two steps of a pair alternate
        for k, leg in legs.items():
            if sum(times[k]) < a.seconds * 1e3 or len(times[k]) < 5:
                times[k].append(timed(leg))
    for k, v in times.items():
        res[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "steps": len(v)}
    res["ratios"] = {"deterministic_over_default_bs%d_%s" % (bs, kind): round(res["deterministic_bs%d_%s" % (bs, kind)]["median_ms"] /
                                                                            res["default_bs%d_%s" % (bs, kind)]["median_ms"], 3)
                     for bs in (32, 256) for kind in ("natural", "noise")}
    try:
        res["kernels_ms_per_step"] = {k: kernel_times(legs[k]) for k in legs}
    except Exception as e:      # noqa: BLE001
        res["kernels_ms_per_step"] = {"unavailable": "%s: %s" % (type(e).__name__, str(e)[:200])}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
