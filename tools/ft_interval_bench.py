#!/usr/bin/env python3
"""The fine-tune step (forward + backward + fused Adam) at the sampling intervals 4, 5 and 6 in ONE process, legs alternating
round-robin, on config 4's batch (bs 256 x 1 x 48 x 48 crops, 2-stage sdy x4):
  1  mulut_amd.finetune.MuLUT          interval 4 (shipped fine-tuned tables)
  2  mulut_amd.finetune.MuLUTInterval  interval 5 (transferred tables of tests/golden/interval_fixtures.npz)
  3  mulut_amd.finetune.MuLUTInterval  interval 6
  4  the same module at interval 5 / 6 as torch operators on the GPU: oracle/ft_torch.forward on device tensors, if it runs there
     unmodified -- what a user without the HIP path could do
on natural crops and, for legs 1-3, on uniform noise (every row of every table touched).  Every leg is warmed up first, then timed
for at least --seconds of device-synchronised steps; medians and min-max per leg.  --kernels adds per-kernel device times of legs 2
and 3 from torch.profiler.   python tools/ft_interval_bench.py --out profiles/ft_interval_bench.json

--modes LIST (default sdy: the legs and the output above, unchanged) with one of the 4 x 4 patterns e, h, o in the list runs legs 1-3 on
mulut_amd.finetune.MuLUTWide with seeded ramp tables (there are no shipped tables of e, h, o), and BESIDE them, in the same round-robin,
legs 1-3 of sdy on the same kind of tables (hip_sdy_interval*): the ratio of the two is what the halo of 3 and the wider taps cost.
    python tools/ft_interval_bench.py --modes eho --kernels --out profiles/ft_wide_bench.json
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
from mulut_amd.finetune import MuLUT, MuLUTInterval, MuLUTWide  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402


def tables(interval):
    if interval == 4:
        return {"s%d_%s" % (s, m): np.load(os.path.join(ROOT, "tests", "golden", "luts", "LUT_ft_x4_4bit_int8_s%d_%s.npy" % (s, m))).reshape(-1, 16 if s == 2 else 1)
                for s in (1, 2) for m in "sdy"}
    fx = np.load(os.path.join(ROOT, "tests", "golden", "interval_fixtures.npz"))
    return {"s%d_%s" % (s, m): fx["iv%d/lut/s%d_%s" % (interval, s, m)].reshape(-1, 16 if s == 2 else 1) for s in (1, 2) for m in "sdy"}


def ramp_tables(interval, modes):
    """Seeded tables for any pattern: a stage returns its input plus noise (the ramp of tests/reach_cases.py), so the second stage sees
    the content the first was given -- smooth crops stay smooth -- and not the mid-grey that random tables collapse to."""
    L, q = 2 ** (8 - interval) + 1, 2 ** interval
    a = (np.arange(L ** 4) // L ** 3)[:, None]
    out = {}
    for s in (1, 2):
        for i, m in enumerate(modes):
            n = np.random.default_rng([interval, s, i]).integers(-40, 41, (L ** 4, 16 if s == 2 else 1))
            out["s%d_%s" % (s, m)] = np.clip((q * a + n) // 4 if s == 2 else q * a - 128 + n, -127, 127)
    return out


def module(interval, modes="sdy", ramp=False):
    with tempfile.TemporaryDirectory() as td:
        for k, t in (ramp_tables(interval, modes) if ramp else tables(interval)).items():
            np.save(os.path.join(td, "LUT_x4_%dbit_int8_%s.npy" % (interval, k)), t.astype(np.int8))
        cls = MuLUTWide if any(m in "eho" for m in modes) else MuLUT if interval == 4 else MuLUTInterval
        return cls(td, 2, modes, upscale=4, interval=interval).cuda()


class HipLeg:
    def __init__(self, interval, x, y, modes="sdy", ramp=False):
        self.net, self.x, self.y = module(interval, modes, ramp), x, y
        self.opt = torch.optim.Adam(self.net.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, fused=True)

    def step(self):
        self.opt.zero_grad()
        loss = torch.nn.functional.mse_loss(self.net(self.x), self.y)
        loss.backward()
        self.opt.step()
        return loss


class TorchLeg:
    """oracle/ft_torch.forward on device tensors (nothing of it is edited: it either runs under torch.device('cuda') or the leg is dropped)."""

    def __init__(self, interval, x, y):
        from oracle import ft_torch
        self.ft, self.interval, self.x, self.y = ft_torch, interval, x, y
        self.w = {k: torch.from_numpy(t.astype(np.float32) / 127.0).cuda().requires_grad_(True) for k, t in tables(interval).items()}
        self.opt = torch.optim.Adam(list(self.w.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, fused=True)

    def step(self):
        self.opt.zero_grad()
        with torch.device("cuda"):
            loss = torch.nn.functional.mse_loss(self.ft.forward(self.w, self.x, 2, "sdy", 4, self.interval), self.y)
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
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--crop", type=int, default=48)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per leg, at least")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", default=None, help="run --steps steps of this one leg and stop (for a profiler): e.g. hip_interval6_natural")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--modes", default="sdy", help="a list with e, h or o: MuLUTWide on seeded ramp tables, with sdy on such tables beside it")
    a = ap.parse_args()
    wide = any(m in "eho" for m in a.modes)
    if a.modes != "sdy" and not wide:
        ap.error("--modes takes sdy or a list with one of e, h, o")
    g = torch.Generator(device="cuda").manual_seed(0)
    big = natural_frames(1, 1080, 1920, 1, 0)[0, :, :, 0]
    rng = np.random.default_rng(0)
    ys, xs = rng.integers(0, 1080 - a.crop, a.bs), rng.integers(0, 1920 - a.crop, a.bs)
    data = {"natural": torch.from_numpy(np.stack([big[p:p + a.crop, q:q + a.crop] for p, q in zip(ys, xs)])[:, None].astype(np.float32) / 255.0).cuda(),
            "noise": torch.randint(0, 256, (a.bs, 1, a.crop, a.crop), device="cuda", generator=g).float() / 255.0}
    y = torch.rand((a.bs, 1, a.crop * 4, a.crop * 4), device="cuda", generator=g)
    res = {"metric": "LUT fine-tune step (fwd+bwd+Adam), 2-stage %s x4, ms per step" % a.modes, "batch": a.bs, "crop": a.crop,
           "source_hash": _native.source_hash(), "device": torch.cuda.get_device_name(0)}
    if a.only:
        kind = a.only.rsplit("_", 1)[1]
        leg = HipLeg(int(a.only[len("hip_interval")]), data[kind], y, a.modes, wide) if a.only.startswith("hip_interval") else \
            HipLeg(int(a.only[len("hip_sdy_interval")]), data[kind], y, "sdy", True)
        for _ in range(a.steps):
            leg.step()
        torch.cuda.synchronize()
        return
    legs = {}
    for kind in ("natural", "noise"):
        for iv in (4, 5, 6):
            legs["hip_interval%d_%s" % (iv, kind)] = HipLeg(iv, data[kind], y, a.modes, wide)
            if wide:
                legs["hip_sdy_interval%d_%s" % (iv, kind)] = HipLeg(iv, data[kind], y, "sdy", True)
    for iv in () if wide else (5, 6):
        name = "torch_ops_interval%d_natural" % iv
        try:
            leg = TorchLeg(iv, data["natural"], y)
            leg.step()
            torch.cuda.synchronize()
            legs[name] = leg
        except Exception as e:      # noqa: BLE001  (recorded, the leg is dropped)
            res[name] = {"dropped": "%s: %s" % (type(e).__name__, str(e)[:300])}
    for leg in legs.values():      # warm-up of every leg first
        for _ in range(3):
            leg.step()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    while any(sum(v) < a.seconds * 1e3 or len(v) < 5 for v in times.values()):      # round-robin
        for k, leg in legs.items():
            if sum(times[k]) < a.seconds * 1e3 or len(times[k]) < 5:
                times[k].append(timed(leg))
    for k, v in times.items():
        res[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "steps": len(v)}
    med = lambda k: res[k]["median_ms"]      # noqa: E731
    ratios = {}
    for kind in ("natural", "noise"):
        for iv in (5, 6):
            ratios["interval%d_over_interval4_%s" % (iv, kind)] = round(med("hip_interval%d_%s" % (iv, kind)) / med("hip_interval4_%s" % kind), 4)
    for iv in (5, 6):
        if "torch_ops_interval%d_natural" % iv in times:
            ratios["torch_ops_over_hip_interval%d_natural" % iv] = round(med("torch_ops_interval%d_natural" % iv) / med("hip_interval%d_natural" % iv), 2)
    l1 = res["hip_interval4_natural"]
    ratios["interval4_own_spread_natural"] = round(l1["max_ms"] / l1["median_ms"], 4)
    if wide:
        for kind in ("natural", "noise"):
            for iv in (4, 5, 6):
                ratios["%s_over_sdy_interval%d_%s" % (a.modes, iv, kind)] = round(med("hip_interval%d_%s" % (iv, kind)) / med("hip_sdy_interval%d_%s" % (iv, kind)), 4)
    res["ratios"] = ratios
    if a.kernels:
        try:
            names = ["hip_interval4_natural", "hip_interval5_natural", "hip_interval6_natural"]
            names += ["hip_sdy_interval%d_natural" % iv for iv in (4, 5, 6)] if wide else []
            res["kernels_ms_per_step"] = {k: kernel_times(legs[k]) for k in names}
        except Exception as e:      # noqa: BLE001
            res["kernels_ms_per_step"] = {"unavailable": "%s: %s" % (type(e).__name__, str(e)[:200])}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
