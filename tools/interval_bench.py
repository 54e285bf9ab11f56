#!/usr/bin/env python3
"""Sampling intervals 4, 5 and 6 on the same work: 2-stage sdy x4 at P1 (LR 1080 x 1920 x 3, 8 frames per pipeline call), on
D-natural and D-noise frames, all six legs in one process, interleaved call by call.

Tables are seeded synthetic ones of each interval's row count (the kernels' work does not depend on table values, only on the
image content through the interval-4 routes).  After a warm-up, every leg is timed --reps times (one hipEvent pair around one
pipeline call each, the legs alternating); the median gives ms per frame and GHRpix/s (output pixels per second).  Also reported:
each stage's main kernel alone (mulut_last_kernel_ms) and the kernel names.  The last line is one JSON object; --out writes it to a
file as well, with the build's source hash.

    python tools/interval_bench.py [--frames 8] [--reps 21] [--out profiles/interval_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mulut_amd import MuLUTEngine, _native, synthetic_lut  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402

STAGES, MODES, SCALE = 2, "sdy", 4


def make_engine(interval):
    e = MuLUTEngine(0).configure(STAGES, MODES, SCALE, interval)
    e.set_lut_dict({"s%d_%s" % (s + 1, m): synthetic_lut(31 * s + ord(m), SCALE * SCALE if s + 1 == STAGES else 1, interval)
                    for s in range(STAGES) for m in MODES})
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    H, W, F = 1080, 1920, opt.frames
    inputs = {"natural": torch.from_numpy(natural_frames(F, H, W, 3, seed=0)).cuda(),
              "noise": torch.from_numpy(np.random.default_rng(0).integers(0, 256, (F, H, W, 3), dtype=np.uint8)).cuda()}
    out = torch.empty((F, H * SCALE, W * SCALE, 3), dtype=torch.uint8, device="cuda")
    engines = {iv: make_engine(iv) for iv in (4, 5, 6)}
    legs = [(iv, d) for d in ("natural", "noise") for iv in (4, 5, 6)]
    for _ in range(opt.warmup):
        for iv, d in legs:
            engines[iv].pipeline(inputs[d], out=out)
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(opt.reps):
        for iv, d in legs:
            ev0.record()
            engines[iv].pipeline(inputs[d], out=out)
            ev1.record()
            ev1.synchronize()
            times[(iv, d)].append(ev0.elapsed_time(ev1))
    rows = {}
    hr_pixels = F * H * SCALE * W * SCALE
    for iv, d in legs:
        e = engines[iv]
        e.set_stage_timing(True)
        e.pipeline(inputs[d], out=out)
        kernel_ms = [float(v) for v in e.last_kernel_ms()]
        e.set_stage_timing(False)
        med = statistics.median(times[(iv, d)])
        rows["iv%d_%s" % (iv, d)] = {"interval": iv, "data": d, "ms_per_frame": med / F, "ghrpix_per_s": hr_pixels / (med * 1e-3) / 1e9,
                                     "ms_per_call_min": min(times[(iv, d)]), "ms_per_call_max": max(times[(iv, d)]),
                                     "stage_kernel_ms": kernel_ms, "kernels": [e.kernel_name(False), e.kernel_name(True)]}
        print("interval %d %-8s %8.3f ms/frame  %7.3f GHRpix/s  (min %.3f max %.3f ms/call)  stage kernels %s ms  %s" % (
            iv, d, med / F, rows["iv%d_%s" % (iv, d)]["ghrpix_per_s"], min(times[(iv, d)]), max(times[(iv, d)]),
            ", ".join("%.3f" % v for v in kernel_ms), " + ".join(rows["iv%d_%s" % (iv, d)]["kernels"])), flush=True)
    ratios = {}
    for d in ("natural", "noise"):
        for iv in (5, 6):
            ratios["iv%d_over_iv4_throughput_%s" % (iv, d)] = rows["iv%d_%s" % (iv, d)]["ghrpix_per_s"] / rows["iv4_%s" % d]["ghrpix_per_s"]
    for e in engines.values():
        e.close()
    res = {"tool": "interval_bench", "source_hash": _native.source_hash(), "frames": F, "shape": [H, W, 3], "scale": SCALE,
           "stages": STAGES, "modes": MODES, "reps": opt.reps, "legs": rows, "throughput_ratios": ratios}
    line = json.dumps(res)
    if opt.out:
        with open(opt.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
