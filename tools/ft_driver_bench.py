#!/usr/bin/env python3
"""The fine-tune DRIVER loop (mulut_amd.finetune_lut.finetune: data + step, as a user runs it) with the batches cut on the host
(CropProvider, --hostData) and on the device (DeviceCropProvider, the default), in ONE process, runs of the two alternating, at
bs 32 and bs 256, crop 48, 2-stage sdy x4, on 8 synthetic 340 x 510 / 1360 x 2040 RGB pairs written to a temporary directory.

A run is three display intervals; what is reported is the wall time per iteration between two display points (the driver's rT, taken
here from the clock at its log calls: the log line rounds rT to 0.1 ms) of the second and third -- the first holds the warm-up.  Beside it, in the same process:
  step_alone_ms     the step (forward + backward + the driver's Adam) on one fixed device batch, steps queued back to back
  crop_kernel_ms    device-event time of mulut_ft_crop_batch alone (draws already on the device), launches back to back
  fill_ms           device-event time of a plain fill of the same two output tensors, measured in rounds alternating with the kernel's
    python tools/ft_driver_bench.py --out profiles/ft_driver_ab.json
Exits 1 if device data is slower than host data at either batch size (the one hard condition)."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mulut_amd import _native, finetune_lut  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402

SCALE, CROP = 4, 48


def write_pairs(root, n):
    os.makedirs(os.path.join(root, "HR"))
    os.makedirs(os.path.join(root, "LR", "X4"))
    for k in range(n):
        hr = natural_frames(1, 1360, 2040, 3, 100 + k)[0]
        lr = hr.reshape(340, 4, 510, 4, 3).astype(np.float32).mean(axis=(1, 3)).round().astype(np.uint8)
        Image.fromarray(hr).save(os.path.join(root, "HR", "%04d.png" % (k + 1)), compress_level=1)
        Image.fromarray(lr).save(os.path.join(root, "LR", "X4", "%04dx4.png" % (k + 1)), compress_level=1)


def write_tables(exp):
    os.makedirs(exp)
    for s in (1, 2):
        for m in "sdy":
            name = "x4_4bit_int8_s%d_%s.npy" % (s, m)
            np.save(os.path.join(exp, "LUT_" + name), np.load(os.path.join(ROOT, "tests", "golden", "luts", "LUT_ft_" + name)))


def driver_run(train, exp, bs, host, per_interval):
    """One finetune() call of 3 display intervals -> ms per iteration of the second and third."""
    stamps = []

    def log(line):
        if "rT:" in line:
            stamps.append(time.perf_counter())

    opt = finetune_lut.build_parser().parse_args(["--stages", "2", "--modes", "sdy", "-e", exp, "--trainDir", train, "--batchSize", str(bs),
                                                  "--cropSize", str(CROP), "--totalIter", str(3 * per_interval), "--displayStep", str(per_interval),
                                                  "--valStep", "0", "--seed", "0"] + (["--hostData"] if host else []))
    finetune_lut.finetune(opt, log=log)
    assert len(stamps) == 3
    return [(b - a) * 1e3 / per_interval for a, b in zip(stamps, stamps[1:])]


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernel_and_fill(train, bs, rounds=15, reps=20):
    lib = _native.load()
    prov = finetune_lut.DeviceCropProvider(train, SCALE, CROP, bs, seed=1)
    draws = torch.from_numpy(prov.draw()).cuda()
    im, lb = prov.next()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():
        rc = lib.mulut_ft_crop_batch(0, prov.pool.data_ptr(), prov.pool_bytes, prov.table.data_ptr(), len(prov.shapes), draws.data_ptr(), bs, CROP, SCALE,
                                     im.data_ptr(), lb.data_ptr(), prov.bad.data_ptr(), st)
        assert rc == 0

    def fill():
        im.fill_(0.5)
        lb.fill_(0.5)

    for fn in (kernel, fill):
        events_ms(fn, reps)
    k, f = [], []
    for _ in range(rounds):
        k.append(events_ms(kernel, reps))
        f.append(events_ms(fill, reps))
    assert int(prov.bad.item()) == 0
    out_bytes = (im.numel() + lb.numel()) * 4
    return {"crop_kernel_ms": round(float(np.median(k)), 5), "crop_kernel_min_max_ms": [round(min(k), 5), round(max(k), 5)],
            "fill_ms": round(float(np.median(f)), 5), "fill_min_max_ms": [round(min(f), 5), round(max(f), 5)],
            "kernel_over_fill": round(float(np.median(k) / np.median(f)), 3), "output_bytes": out_bytes,
            "crop_kernel_output_GBps": round(out_bytes / np.median(k) / 1e6, 1)}, (im, lb)


def step_alone(exp, batch, steps):
    from mulut_amd.finetune import Adam, MuLUT
    net = MuLUT(exp, 2, list("sdy"), upscale=SCALE, interval=4).cuda()
    optim = Adam([p for p in net.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)      # the driver's
    im, lb = batch

    def step():
        optim.zero_grad()
        torch.nn.functional.mse_loss(net(im), lb).backward()
        optim.step()

    events_ms(step, 5)
    v = [events_ms(step, steps) for _ in range(5)]
    return {"step_alone_ms": round(float(np.median(v)), 4), "step_alone_min_max_ms": [round(min(v), 4), round(max(v), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2, help="runs of each provider per batch size, alternating")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "LUT fine-tune driver loop, 2-stage sdy x4, crop 48: ms per iteration (wall time between display points, the driver's rT)",
           "pairs": "%d synthetic 340x510 / 1360x2040 RGB" % a.pairs, "source_hash": _native.source_hash(), "device": torch.cuda.get_device_name(0)}
    slower = []
    with tempfile.TemporaryDirectory() as td:
        train, exp = os.path.join(td, "train"), os.path.join(td, "exp")
        write_pairs(train, a.pairs)
        write_tables(exp)
        for bs in (32, 256):
            # iterations per display interval: about a second of wall time each (host data at bs 256 takes tens of ms per iteration)
            per = {"device": 300, "host": 300 if bs == 32 else 40}
            rt = {"device": [], "host": []}
            for _ in range(a.rounds):
                for name in ("host", "device"):
                    rt[name] += driver_run(train, exp, bs, name == "host", per[name])
            r = {"%s_data_ms_per_iter" % n: round(float(np.median(v)), 4) for n, v in rt.items()}
            r.update({"%s_data_min_max_ms" % n: [round(min(v), 4), round(max(v), 4)] for n, v in rt.items()})
            r["iterations_per_interval"] = per
            r["host_over_device"] = round(r["host_data_ms_per_iter"] / r["device_data_ms_per_iter"], 2)
            kf, batch = kernel_and_fill(train, bs)
            r.update(kf)
            r.update(step_alone(exp, batch, 100))
            r["device_loop_over_step_alone"] = round(r["device_data_ms_per_iter"] / r["step_alone_ms"], 3)
            res["bs%d" % bs] = r
            if r["device_data_ms_per_iter"] > r["host_data_ms_per_iter"]:
                slower.append(bs)
    res["device_data_not_slower_than_host_data"] = not slower
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(1 if slower else 0)


if __name__ == "__main__":
    main()
