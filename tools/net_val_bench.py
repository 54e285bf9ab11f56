#!/usr/bin/env python3
"""What a validation point costs the thread that drives network training (mulut_amd.train_model), on the host loop (net_valid_steps,
the reference's) and from a device-resident set (--valResident: NetValSet, resident_net_valid_steps), in ONE process, on the shipped
nf-64 x4 sdy weights (tests/golden/Model_200000.pth).

  sets     Set5 (tests/golden/Set5, the real images) and a synthetic set of --images natural-like frames of mulut_amd.synth at
           Urban100's size class: HR 1024 x 768, LR 256 x 192 (the HR's 4 x 4 box means).
  1. stall   wall time by which one validation point holds up the loop: the device is idle at the start, the clock stops when the call
             returns.  net_valid_steps and the resident path at each --valSave alternate, medians of --rounds rounds behind one warm-up
             round, with minimum and maximum.  The points are at iteration 2000, so the host loop writes _net, _input and _gt of
             every image at every point; the resident path wrote _input and _gt with its first point (the warm-up round).  For the
             resident path with files, `files_done_after_ms` is the time from the call's return until the point's last PNG is on disk.
  2. launch  the list form alone (NetPlan.run: `stages` launches for the whole set, HWC pool to HWC pool) against the per-image loop
             on the same pools with everything preallocated: HWC to planar, NetEngine.stage(out=) per stage, planar to HWC into the
             image's slot.  Wall time including the launches, the device idle at both ends.
    python tools/net_val_bench.py --out profiles/net_val_bench.json
`verdict` says, per set, whether each resident mode's slowest round beat net_valid_steps' fastest, and whether the list launch's
slowest round beat the per-image loop's fastest.  Always exits 0 when the two paths agree on the files' bytes: there is no number to meet."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mulut_amd import _native, network  # noqa: E402
from mulut_amd.net_engine import NetEngine  # noqa: E402
from mulut_amd.net_val import NetValSet, net_valid_steps, resident_net_valid_steps  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402

SCALE, IT = 4, 2000
GOLDEN = os.path.join(ROOT, "tests", "golden")


def write_urban_like(root, n, H=768, W=1024):
    hr_dir, lr_dir = os.path.join(root, "Urban100", "HR"), os.path.join(root, "Urban100", "LR_bicubic", "X4")
    os.makedirs(hr_dir)
    os.makedirs(lr_dir)

    def one(k):
        hr = natural_frames(1, H, W, 3, 2000 + k)[0]
        lr = hr.reshape(H // 4, 4, W // 4, 4, 3).astype(np.float32).mean(axis=(1, 3)).round().astype(np.uint8)
        Image.fromarray(hr).save(os.path.join(hr_dir, "img_%03d.png" % (k + 1)), compress_level=1)
        Image.fromarray(lr).save(os.path.join(lr_dir, "img_%03d.png" % (k + 1)), compress_level=1)
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(one, range(n)))
    return {"images": n, "hr_size": [H, W], "lr_size": [H // 4, W // 4]}


def spread(v):
    return {"median_ms": round(float(np.median(v)), 2), "min_max_ms": [round(min(v), 2), round(max(v), 2)]}


def tree(root):
    out = {}
    for d, _, fs in os.walk(root):
        for fn in fs:
            with open(os.path.join(d, fn), "rb") as f:
                out[os.path.relpath(os.path.join(d, fn), root)] = f.read()
    return out


def stall(eng, val, debug, td, tag, rounds, workers):
    quiet = lambda line: None  # noqa: E731
    opts = {name: argparse.Namespace(valDir=val, valoutDir=os.path.join(td, "out_%s_%s" % (tag, name)), scale=SCALE, debug=debug, valSave=name,
                                     totalIter=IT, valStep=IT) for name in ("host", "every", "last", "never")}
    t0 = time.perf_counter()
    vsets = {name: NetValSet(opts[name], workers=workers) for name in ("every", "last", "never")}      # (one each: a set writes _input / _gt once)
    torch.cuda.synchronize()
    build_s = (time.perf_counter() - t0) / 3
    times, behind, results = {name: [] for name in opts}, {"every": [], "last": []}, {}
    for r in range(rounds + 1):                         # (round 0 is the warm-up)
        for name, opt in opts.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "host":
                res = net_valid_steps(eng, opt, IT, quiet)
            else:
                res = resident_net_valid_steps(eng, vsets[name], opt, IT, quiet)
            t1 = time.perf_counter()
            if name != "host":
                vsets[name].join()
            t2 = time.perf_counter()
            results[name] = res
            print("# %s round %d %s: %.1f ms, files done %.1f ms after" % (tag, r, name, (t1 - t0) * 1e3, (t2 - t1) * 1e3), file=sys.stderr, flush=True)
            if r:
                times[name].append((t1 - t0) * 1e3)
                if name in behind:
                    behind[name].append((t2 - t1) * 1e3)
    host_tree = tree(opts["host"].valoutDir)
    same_files = all(tree(opts[name].valoutDir) == host_tree for name in ("every", "last"))
    psnr_gap = max(float(np.abs(np.asarray(results["host"][ds], np.float64) - results[name][ds]).max()) for name in vsets for ds in results["host"])
    vs = vsets["every"]
    out = {"set_bytes_on_device": vs.nbytes, "set_build_s": round(build_s, 2), "images": len(vs.shapes), "files_of_a_host_point": len(host_tree),
           "same_files_as_net_valid_steps": same_files, "largest_psnr_difference_db": psnr_gap, "net_valid_steps": spread(times["host"])}
    for name in ("every", "last", "never"):
        out["resident_save_" + name] = spread(times[name])
        if name in behind:
            out["resident_save_" + name]["files_done_after_ms"] = spread(behind[name])
        out["resident_save_" + name]["net_valid_steps_over_resident"] = round(float(np.median(times["host"]) / np.median(times[name])), 1)
    ok = {name: bool(max(times[name]) < min(times["host"])) for name in ("every", "last", "never")}
    launch_out, launch_ok = launch(eng, vs, rounds)
    for v in vsets.values():
        v.close()
    return out, launch_out, ok, launch_ok, same_files


def launch(eng, vset, rounds):
    """NetPlan.run per dataset against the per-image stage loop, on vset's pools."""
    plans = vset.plans(eng)
    bufs = []
    for sh in vset.shapes:
        bufs.append((torch.empty((1, 3, sh.h, sh.w), dtype=torch.uint8, device="cuda"),
                     [torch.empty((1, 3, sh.h * (SCALE if s == eng.stages else 1), sh.w * (SCALE if s == eng.stages else 1)), dtype=torch.uint8, device="cuda")
                      for s in range(1, eng.stages + 1)]))

    def as_list():
        for p in plans:
            p.run(vset.lr_pool, vset.out_pool)

    def per_image():
        for n, sh in enumerate(vset.shapes):
            x, outs = bufs[n]
            x[0].copy_(vset.lr_bytes_hwc(n).permute(2, 0, 1))
            for s in range(1, eng.stages + 1):
                x = eng.stage(s, x, out=outs[s - 1])
            vset.out_slot(n).view(sh.H, sh.W, 3).copy_(x[0].permute(1, 2, 0))

    t_list, t_each, kept = [], [], {}
    for r in range(rounds + 1):
        for name, fn, acc in (("list", as_list, t_list), ("per_image", per_image, t_each)):
            vset.out_pool.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                acc.append((time.perf_counter() - t0) * 1e3)
            kept[name] = vset.out_pool.clone()
    same = bool(torch.equal(kept["list"], kept["per_image"]))
    out = {"list_launch": spread(t_list), "per_image_stage_loop": spread(t_each), "images": len(vset.shapes), "launches_of_the_list": eng.stages * len(plans),
           "launches_of_the_loop": eng.stages * len(vset.shapes), "same_bytes": same,
           "per_image_over_list": round(float(np.median(t_each) / np.median(t_list)), 2)}
    return out, bool(max(t_list) < min(t_each)) and same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100, help="images of the synthetic Urban100-like set")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "one validation point of network training, nf-64 2-stage sdy x4: wall ms by which it holds up the training thread",
           "source_hash": _native.source_hash(), "device": torch.cuda.get_device_name(0), "val_workers": a.workers, "rounds": a.rounds, "iteration": IT,
           "sets": {}, "verdict": {}}
    eng = NetEngine(network.load_checkpoint(os.path.join(GOLDEN, "Model_200000.pth")))
    agree = True
    with tempfile.TemporaryDirectory() as td:
        synth = os.path.join(td, "bench")
        shape = write_urban_like(synth, a.images)
        for tag, val, debug, about in (("Set5", GOLDEN, True, {"images": 5, "source": "tests/golden/Set5"}), ("urban_like", synth, False, shape)):
            stall_out, launch_out, ok, launch_ok, same_files = stall(eng, val, debug, td, tag, a.rounds, a.workers)
            res["sets"][tag] = dict(about, stall=stall_out, launch=launch_out)
            res["verdict"][tag] = {"resident_slowest_round_beats_host_fastest": ok, "list_slowest_round_beats_loop_fastest": launch_ok}
            agree = agree and same_files and launch_out["same_bytes"]
            if a.out:                                   # (after every set: a run that is cut short leaves what it finished)
                with open(a.out, "w") as f:
                    f.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if agree else 1)


if __name__ == "__main__":
    main()
