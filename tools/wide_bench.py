#!/usr/bin/env python3
"""The 4 x 4 patterns against the 3 x 3 ones on the same work: 8 natural 1080p frames, 2 stages, x4, in one process, legs alternated.

  (a) sdy, forced to the full-table kernels (first_stage_kernel 2: stage_u1w_kernel; final_stage_kernel 1: stage_up_kernel)
  (b) eho on the same two kernel templates instantiated with a 3-px halo (mulut_kernel_name: stage_wide1_kernel, stage_wide_up_kernel<4>)

Both legs make the same number of passes (3 modes x 4 rotations per site and stage), with seeded synthetic tables.  Per leg and
round: ms per frame of the whole pipeline call (after a warm-up, timed over more than a second of calls) and the per-stage time of
each stage's main kernel (mulut_last_kernel_ms).  The last line is one JSON object with every round.

    python tools/wide_bench.py [--frames 8] [--rounds 3] [--min-seconds 1.5]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from mulut_amd import MuLUTEngine, synthetic_lut  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402

LEGS = {"a_sdy_full_table": ("sdy", {"first_stage_kernel": 2, "final_stage_kernel": 1}), "b_eho_wide": ("eho", {})}


def make_engine(modes, tuning, stages=2, scale=4):
    e = MuLUTEngine(0).configure(stages, modes, scale, 4)
    e.set_lut_dict({"s%d_%s" % (s + 1, m): synthetic_lut(31 * s + ord(m), scale * scale if s + 1 == stages else 1)
                    for s in range(stages) for m in modes})
    for k, v in tuning.items():
        e.set_tuning(k, v)
    return e


def time_leg(e, x, out, min_seconds):
    """ms per call: repeat until the timed loop lasts longer than min_seconds"""
    n = 1
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            e.pipeline(x, out=out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt * 1e3 / n
        n = max(n * 2, int(n * min_seconds * 1.2 / max(dt, 1e-6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=1.5)
    opt = ap.parse_args()
    frames = natural_frames(opt.frames, 1080, 1920, 3, seed=0)
    x = torch.from_numpy(frames).cuda()
    out = torch.empty((opt.frames, 4320, 7680, 3), dtype=torch.uint8, device="cuda")
    engines = {name: make_engine(modes, tuning) for name, (modes, tuning) in LEGS.items()}
    for e in engines.values():          # warm-up (first launches set kernel attributes), then one untimed pass
        e.pipeline(x, out=out)
        e.pipeline(x, out=out)
    torch.cuda.synchronize()
    rounds = []
    for r in range(opt.rounds):
        row = {}
        for name, e in engines.items():
            ms = time_leg(e, x, out, opt.min_seconds)
            e.set_stage_timing(True)
            e.pipeline(x, out=out)
            kernel_ms = [float(v) for v in e.last_kernel_ms()]
            e.set_stage_timing(False)
            row[name] = {"ms_per_frame": ms / opt.frames, "stage_kernel_ms": kernel_ms,
                         "kernels": [e.kernel_name(False), e.kernel_name(True)]}
            print("round %d  %-18s %8.3f ms/frame   stage kernels %s ms (%d frames)" % (
                r, name, ms / opt.frames, ", ".join("%.3f" % v for v in kernel_ms), opt.frames), flush=True)
        a, b = row["a_sdy_full_table"], row["b_eho_wide"]
        row["ratio_b_over_a"] = {"pipeline": b["ms_per_frame"] / a["ms_per_frame"],
                                 "stages": [kb / ka if ka > 0 else None for ka, kb in zip(a["stage_kernel_ms"], b["stage_kernel_ms"])]}
        print("round %d  ratio b/a: pipeline %.3f, stages %s" % (
            r, row["ratio_b_over_a"]["pipeline"], ", ".join("%.3f" % v for v in row["ratio_b_over_a"]["stages"] if v is not None)), flush=True)
        rounds.append(row)
    for e in engines.values():
        e.close()
    print(json.dumps({"tool": "wide_bench", "frames": opt.frames, "shape": [1080, 1920, 3], "scale": 4, "stages": 2,
                      "rounds": rounds}))


if __name__ == "__main__":
    main()
