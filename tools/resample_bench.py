#!/usr/bin/env python3
"""The resample kernel against a plain copy (needs the GPU).

  tools/resample_bench.py [--out profiles/resample_bench.json]

mulut_resample_run moves `in + out` bytes once, so it is judged as a copy: per case the kernel (device-event time, the plan made
beforehand) and a device-to-device copy of (in + out) / 2 bytes -- the same bytes read plus written -- are timed in ONE process in
rounds alternating between the two, medians reported:
  down4   a 1356 x 2040 x 3 frame (a DIV2K image's size) to 339 x 510, HWC: what make_lr and --makeLR run
  up4     1080 x 1920 x 3 to 4320 x 7680, HWC: what test_lut --bicubicBaseline runs, at a 4K-class output
Both results are checked against Pillow before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mulut_amd import _native  # noqa: E402
from mulut_amd.resample import bicubic  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402

CASES = [("down4", 1356, 2040, 339, 510), ("up4", 1080, 1920, 4320, 7680)]


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def one_case(name, h, w, oh, ow, rounds, reps):
    frame = natural_frames(1, h, w, 3, seed=2)[0]
    x = torch.from_numpy(frame).cuda()
    out = torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda")
    bicubic(x, (oh, ow), out=out)
    want = np.array(Image.fromarray(frame).resize((ow, oh), resample=Image.BICUBIC))
    assert np.array_equal(out.cpu().numpy(), want), name
    moved = x.numel() + out.numel()
    src = torch.randint(0, 256, (moved // 2,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def kernel():
        bicubic(x, (oh, ow), out=out)

    def copy():
        dst.copy_(src)

    for fn in (kernel, copy):
        events_ms(fn, reps)
    k, c = [], []
    for _ in range(rounds):
        k.append(events_ms(kernel, reps))
        c.append(events_ms(copy, reps))
    km, cm = float(np.median(k)), float(np.median(c))
    return {"case": name, "in": [h, w, 3], "out": [oh, ow, 3], "bytes_moved": moved,
            "kernel_ms": round(km, 5), "kernel_min_max_ms": [round(min(k), 5), round(max(k), 5)],
            "copy_ms": round(cm, 5), "copy_min_max_ms": [round(min(c), 5), round(max(c), 5)],
            "kernel_over_copy": round(km / cm, 3), "kernel_GBps": round(moved / km / 1e6, 1), "copy_GBps": round(moved / cm / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"tool": "tools/resample_bench.py", "device": torch.cuda.get_device_name(0), "source_hash": _native.source_hash(),
           "rounds": args.rounds, "reps": args.reps, "cases": [one_case(*c, args.rounds, args.reps) for c in CASES]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
