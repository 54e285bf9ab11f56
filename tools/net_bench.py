#!/usr/bin/env python3
"""The fused network forward against the torch operators it replaces, on the same weights (the shipped checkpoint, nf 64, sdy, x4).

    python tools/net_bench.py [--rounds 7] [--out profiles/net_bench.json]

What is compared: `NetEngine` (mulut_net_table / mulut_net_stage, one kernel per call) and `network.SRNets` run through torch on the
GPU, as the parent tree does the same work: `transfer_to_lut.transfer_one` in its 100 chunks for a table, and for a stage of
`mulut_predict` the twelve rotate / pad / forward / rotate-back / round passes over the image in bands of rows (a whole 1080 x 1920 x 3
pass is 6.2 M sites x 320 floats of activations per layer; the bands keep a pass at about a million sites, as transfer_one's chunks do).
  (a) one interval-4 table, stage 2 (u = 4): to a host array, as transfer() needs it, and the fused kernel alone on the device;
  (b) stage 2 of predict (the upscaling stage) on 270 x 480 x 3 and 1080 x 1920 x 3, device to device.
Each round times every variant once, alternating, after a warm-up of each shape; a time is a host clock around work that ends in a
device synchronise.  Reported: median, minimum and maximum per variant, the ratio of the medians, and for the fused calls the FLOP/s
the algorithm needs (2 x 46,336 multiply-adds per site at nf 64, u 4 -- padding not counted) over the median, as a share of the
157.3 TFLOP/s that MI355X_MICROARCH.md gives for the f32-input MFMA.  The results of both paths are compared first (the bar of
tests/net_cases.py).  There is no CPU path: without a GPU this fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mulut_amd import _native, network, transfer_to_lut as T      # noqa: E402
from mulut_amd.net_engine import NetEngine      # noqa: E402

PEAK_F32_MFMA = 157.3e12
BYTE = torch.arange(256, dtype=torch.float32) / 255.0


def site_flops(nf, u):
    return 2 * (4 * nf + nf * nf * (1 + 2 + 3 + 4) + 5 * nf * u * u)


def torch_stage(net, x_u8, modes, stage, is_last, band_sites=1 << 20):
    """One stage of mulut_predict('valid') through torch: the passes of sr/1_train_model.py:31-35 with the forward run over bands of
    rows of the rotated, padded image, then the stage's average / bias / round / clip."""
    import torch.nn.functional as F
    M = len(modes)
    xf = BYTE.to(x_u8.device)[x_u8.long()]
    pred = None
    for mode in modes:
        pad = network.TAPS[mode.upper()][0] - 1
        for r in range(4):
            xr = F.pad(torch.rot90(xf, r, [2, 3]), (0, pad, 0, pad), mode="replicate")
            N, C, Hp, Wp = xr.shape
            rows = max(1, band_sites // (N * C * (Wp - pad)))
            bands = [net(xr[:, :, y:min(y + rows, Hp - pad) + pad], stage=stage, mode=mode) for y in range(0, Hp - pad, rows)]
            y = torch.round(torch.rot90(torch.cat(bands, 2), (4 - r) % 4, [2, 3]) * 127)
            pred = y if pred is None else pred + y
    if is_last:
        return torch.clamp(torch.round(pred / M), 0, 255).to(torch.uint8)
    return torch.round(torch.clamp(pred / (4 * M) + 127, 0, 255)).to(torch.uint8)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def compare(variants, rounds):
    """{name: fn} -> {name: {median_ms, min_ms, max_ms, times_ms}}: a warm-up of each, then `rounds` rounds of each once, alternating."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "times_ms": [round(t, 4) for t in v]} for k, v in times.items()}


def share_off(a, b):
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    return int(d.max()), float((d != 0).float().mean())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_bench.json"))
    ap.add_argument("--checkpoint", default=os.path.join(ROOT, "tests", "golden", "Model_200000.pth"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("net_bench.py: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    nf, u, modes = 64, 4, "sdy"
    net = network.SRNets(nf=nf, scale=4, modes=list(modes), stages=2)
    net.load_state_dict(network.load_checkpoint(args.checkpoint).state_dict(), strict=True)
    eng = NetEngine(net, 0)
    net = net.to(dev).eval()
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _native.source_hash(), "rounds": args.rounds, "model": "Model_200000.pth: nf 64, sdy, x4",
              "peak_f32_mfma_tflops": PEAK_F32_MFMA / 1e12, "flops_per_site": site_flops(nf, u), "cases": {}}
    opt = type("Opt", (), {"interval": 4})()
    with torch.no_grad():
        # ---- (a) one table
        a, b = eng.table(2, "y", 4), torch.from_numpy(T.transfer_one(net, opt, 2, "y", dev)).to(dev)
        worst, share = share_off(a, b)
        r = compare({"fused_to_host": lambda: eng.table(2, "y", 4).cpu().numpy(), "torch_to_host": lambda: T.transfer_one(net, opt, 2, "y", dev),
                     "fused_device": lambda: eng.table(2, "y", 4)}, args.rounds)
        flops = 83521 * site_flops(nf, u)
        result["cases"]["table_interval4_s2_y"] = {
            "sites": 83521, "variants": r, "torch_over_fused_to_host": r["torch_to_host"]["median_ms"] / r["fused_to_host"]["median_ms"],
            "fused_device_tflops": flops / r["fused_device"]["median_ms"] / 1e9, "fused_device_share_of_peak": flops / r["fused_device"]["median_ms"] / 1e9 / (PEAK_F32_MFMA / 1e12),
            "values_off_by_one": share, "largest_difference": worst}
        # ---- (b) the upscaling stage of predict
        for H, W in ((270, 480), (1080, 1920)):
            x = torch.from_numpy(np.random.default_rng(H).integers(0, 256, (1, 3, H, W), dtype=np.uint8)).to(dev)
            out = torch.empty((1, 3, H * u, W * u), dtype=torch.uint8, device=dev)
            worst, share = share_off(eng.stage(2, x, out=out), torch_stage(net, x, modes, 2, True))
            r = compare({"fused": lambda: eng.stage(2, x, out=out), "torch": lambda: torch_stage(net, x, modes, 2, True)}, args.rounds)
            sites = 3 * H * W * 4 * len(modes)
            flops = sites * site_flops(nf, u)
            result["cases"]["stage2_%dx%dx3" % (H, W)] = {
                "sites": sites, "variants": r, "torch_over_fused": r["torch"]["median_ms"] / r["fused"]["median_ms"],
                "fused_tflops": flops / r["fused"]["median_ms"] / 1e9, "fused_share_of_peak": flops / r["fused"]["median_ms"] / 1e9 / (PEAK_F32_MFMA / 1e12),
                "bytes_off_by_one": share, "largest_difference": worst}
            print(json.dumps({k: v for k, v in result["cases"]["stage2_%dx%dx3" % (H, W)].items() if k != "variants"}), flush=True)
    slower = [k for k, c in result["cases"].items() if c.get("torch_over_fused", c.get("torch_over_fused_to_host")) < 1.0]
    result["fused_slower_at"] = slower
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {kk: vv for kk, vv in c.items() if kk != "variants"} for k, c in result["cases"].items()}))
    eng.close()
    return result


if __name__ == "__main__":
    main()
