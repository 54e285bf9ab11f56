#!/usr/bin/env python3
"""What a validation point costs the fine-tune loop, on the host loop (valid_steps, the reference's) and from a device-resident set
(--valResident: DeviceValSet, resident_valid_steps), in ONE process, on a synthetic validation set shaped like the five benchmark
sets: natural-like frames of mulut_amd.synth in each set's size class, the LR files made by mulut_amd.resample.make_lr.  The image
counts and sizes are written into the result (--full takes the benchmark's own counts, 5 / 14 / 100 / 100 / 109).

  1. stall        wall time by which one validation point holds up step(): the device is idle at the start, the clock stops when the
                  call returns.  valid_steps and the resident path at each --valSave alternate, medians over --rounds.  For the
                  resident path with files, `files_done_after_ms` is the time from the call's return until the point's last PNG is on
                  disk: the next point joins them, so it waits for whatever of that is left after the iterations in between.
  2. run          finetune() end to end both ways: --totalIter 4000 --valStep 2000 (points at 1, 2000, 4000), bs 32, crop 48.
  3. scorer       mulut_eval_plan_run of every dataset plus ONE read-back against one mulut_eval_y call per image, on the same bytes.
    python tools/ft_val_bench.py --out profiles/ft_val_bench.json
Exits 1 if the resident point (any --valSave) does not stall the loop for less time than valid_steps beyond the spread of the rounds:
its slowest round against valid_steps' fastest."""
import argparse
import ctypes
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
from mulut_amd import _native, finetune_lut  # noqa: E402
from mulut_amd.resample import make_lr  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402

SCALE = 4
# (dataset, images of the benchmark, images here, HR height, HR width): one size per set, of the set's size class
SETS = [("Set5", 5, 5, 344, 512), ("Set14", 14, 14, 480, 500), ("B100", 100, 20, 320, 480), ("Urban100", 100, 20, 768, 1024),
        ("Manga109", 109, 20, 1168, 824)]


def write_val_sets(root, full):
    jobs = []
    for ds, n_full, n, H, W in SETS:
        os.makedirs(os.path.join(root, ds, "HR"))
        jobs += [(ds, k, H, W) for k in range(n_full if full else n)]

    def one(job):
        ds, k, H, W = job
        Image.fromarray(natural_frames(1, H, W, 3, 1000 + 7 * k + len(ds))[0]).save(os.path.join(root, ds, "HR", "img_%03d.png" % (k + 1)), compress_level=1)
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(one, jobs))
    for ds, _, _, _, _ in SETS:
        make_lr(os.path.join(root, ds, "HR"), os.path.join(root, ds), scales=(SCALE,), layout="benchmark", log=lambda *a: None)
    return {ds: {"images": n_full if full else n, "benchmark_images": n_full, "hr_size": [H, W]} for ds, n_full, n, H, W in SETS}


def write_train(root, n=4):
    os.makedirs(os.path.join(root, "HR"))
    os.makedirs(os.path.join(root, "LR", "X4"))
    for k in range(n):
        hr = natural_frames(1, 680, 1020, 3, 100 + k)[0]
        lr = hr.reshape(170, 4, 255, 4, 3).astype(np.float32).mean(axis=(1, 3)).round().astype(np.uint8)
        Image.fromarray(hr).save(os.path.join(root, "HR", "%04d.png" % (k + 1)), compress_level=1)
        Image.fromarray(lr).save(os.path.join(root, "LR", "X4", "%04dx4.png" % (k + 1)), compress_level=1)


def write_tables(exp):
    os.makedirs(exp)
    for s in (1, 2):
        for m in "sdy":
            name = "x4_4bit_int8_s%d_%s.npy" % (s, m)
            np.save(os.path.join(exp, "LUT_" + name), np.load(os.path.join(ROOT, "tests", "golden", "luts", "LUT_ft_" + name)))


def spread(v):
    return {"median_ms": round(float(np.median(v)), 2), "min_max_ms": [round(min(v), 2), round(max(v), 2)]}


def stall(val, exp, td, rounds, workers):
    from mulut_amd.finetune import MuLUT
    net = MuLUT(exp, 2, list("sdy"), upscale=SCALE, interval=4).cuda()
    quiet = lambda line: None  # noqa: E731
    opts = {name: argparse.Namespace(valDir=val, valoutDir=os.path.join(td, "out_" + name), scale=SCALE, debug=False, valSave=name, totalIter=10, valStep=10)
            for name in ("host", "every", "last", "never")}
    t0 = time.perf_counter()
    vset = finetune_lut.DeviceValSet(opts["every"], workers=workers)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    times = {name: [] for name in opts}
    behind = {"every": [], "last": []}
    results = {}
    for r in range(rounds + 1):                         # (round 0 is the warm-up)
        for name, opt in opts.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "host":
                res = finetune_lut.valid_steps(net, opt, 10, quiet)
            else:
                res = finetune_lut.resident_valid_steps(net, vset, opt, 10, quiet)
            t1 = time.perf_counter()
            vset.join()
            t2 = time.perf_counter()
            results[name] = res
            if r:
                times[name].append((t1 - t0) * 1e3)
                if name in behind:
                    behind[name].append((t2 - t1) * 1e3)
    assert all(results[name] == results["host"] for name in results), "the two paths disagree"
    out = {"set_bytes_on_device": vset.nbytes, "set_build_s": round(build_s, 2), "images": len(vset.shapes),
           "valid_steps": spread(times["host"])}
    for name in ("every", "last", "never"):
        out["resident_save_" + name] = spread(times[name])
        if name in behind:
            out["resident_save_" + name]["files_done_after_ms"] = spread(behind[name])
        out["resident_save_" + name]["valid_steps_over_resident"] = round(float(np.median(times["host"]) / np.median(times[name])), 1)
    vset.close()
    ok = all(max(times[name]) < min(times["host"]) for name in ("every", "last", "never"))
    return out, ok


def run_both(val, train, exp_src, td, iters, workers):
    out = {}
    for name, extra in (("host", []), ("resident_every", ["--valResident", "--valSave", "every"]), ("resident_last", ["--valResident", "--valSave", "last"])):
        exp = os.path.join(td, "run_" + name)
        write_tables(exp)
        opt = finetune_lut.build_parser().parse_args(["--stages", "2", "--modes", "sdy", "-e", exp, "--trainDir", train, "--totalIter", str(iters),
                                                      "--valStep", "2000", "--displayStep", "1000", "--seed", "0", "--valDir", val,
                                                      "--valWorkers", str(workers)] + extra)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        finetune_lut.finetune(opt, log=lambda line: None)
        torch.cuda.synchronize()
        out[name + "_s"] = round(time.perf_counter() - t0, 2)
    out["iterations"], out["validation_points"] = iters, 1 + iters // 2000
    out["host_over_resident_every"] = round(out["host_s"] / out["resident_every_s"], 2)
    out["host_over_resident_last"] = round(out["host_s"] / out["resident_last_s"], 2)
    return out


def scorer(val, td, rounds):
    lib = _native.load()
    opt = argparse.Namespace(valDir=val, valoutDir=os.path.join(td, "out_scorer"), scale=SCALE, debug=False)
    vset = finetune_lut.DeviceValSet(opt, workers=1)
    vset.out_pool.copy_(vset.gt_pool)
    vset.out_pool[::7] += 3                               # something to score
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(max(int(lib.mulut_eval_ws_doubles(H, W)) for _, H, W, _, _, _ in vset.shapes), dtype=torch.float64, device="cuda")
    p, s = ctypes.c_double(), ctypes.c_double()

    def per_image():
        rows = []
        for g, H, W, _, _, _ in vset.shapes:
            assert lib.mulut_eval_y(0, vset.gt_pool.data_ptr() + g, vset.out_pool.data_ptr() + g, H, W, SCALE, ws.data_ptr(), ws.numel(),
                                    ctypes.byref(p), ctypes.byref(s), st) == 0
            rows.append((p.value, s.value))
        return rows

    a, b, t_list, t_each = None, None, [], []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = vset.score()
        t1 = time.perf_counter()
        b = per_image()
        t2 = time.perf_counter()
        if r:
            t_list.append((t1 - t0) * 1e3)
            t_each.append((t2 - t1) * 1e3)
    got = np.concatenate([a[s_["name"]] for s_ in vset.sets])
    same = bool(np.array_equal(got.view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64)))
    vset.close()
    return {"plan_runs_and_one_read_back": spread(t_list), "eval_y_per_image": spread(t_each), "images": len(b), "same_bits": same,
            "per_image_over_list": round(float(np.median(t_each) / np.median(t_list)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true", help="the benchmark's own image counts (328 images)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--skip-run", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "one validation point of the fine-tune driver, 2-stage sdy x4: wall ms by which it holds up step()",
           "source_hash": _native.source_hash(), "device": torch.cuda.get_device_name(0), "val_workers": a.workers, "rounds": a.rounds}
    with tempfile.TemporaryDirectory() as td:
        val, train, exp = os.path.join(td, "bench"), os.path.join(td, "train"), os.path.join(td, "exp")
        res["sets"] = write_val_sets(val, a.full)
        write_train(train)
        write_tables(exp)
        res["stall"], ok = stall(val, exp, td, a.rounds, a.workers)
        res["scorer"] = scorer(val, td, a.rounds)
        if not a.skip_run:
            res["run"] = run_both(val, train, exp, td, a.iters, a.workers)
    res["resident_point_stalls_less_than_valid_steps"] = ok
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok and res["scorer"]["same_bits"] else 1)


if __name__ == "__main__":
    main()
