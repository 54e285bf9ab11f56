#!/usr/bin/env python3
"""One training step of the SR network -- forward, backward and Adam -- on the fused HIP kernels against the torch operators, on the
shipped configuration (nf 64, 2 stages, sdy, x4).

    python tools/net_train_bench.py [--rounds 7] [--batches 8,32,128] [--out profiles/net_train_bench.json]

What is compared: `net_train.NetTrainer.predict` (mulut_net_stage_sum forward, mulut_net_stage_backward backward) and
`net_train.torch_predict` over `network.SRNets` (what `train_model --torchPath` runs), each with its own copy of the same seeded model
and its own `torch.optim.Adam`, on the same random batch [B, 1, 48, 48] with a [B, 1, 192, 192] label, in one process.  Each round
times every variant once, alternating, after a warm-up of each; a time is a host clock around one step that ends in a device
synchronise.  The fused step is also timed with one workspace chunk per pass (`ws_sites` = all sites of a stage, B x 48 x 48: both
stages take a 48 x 48 input) against the default chunk of 64 Ki sites.  At bs 8 and 32 a stage has no more sites than 1.1 x the default
chunk and both workspaces fit the 256 MB Infinity Cache, so that pair only compares one launch pair per pass with two; at bs 128 one
chunk is 294,912 sites, 782 MB, three times the cache, against 4.5 chunks of 176 MB: that pair is the one that measures cache
residency against launch count.  The bytes in the JSON are those of the workspace tensor that was allocated.  Reported: median, minimum and maximum per variant, the ratio
of the medians, whether the gap exceeds the spread (max - min) of either, and the TFLOP/s of the arithmetic a step needs -- 3 x the
forward's FLOPs; the backward's recompute of the forward is overhead, not useful work -- as a share of the 157.3 TFLOP/s of the
f32-input MFMA.  A torch step that does not fit the device is recorded as such.  There is no CPU path: without a GPU this fails.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mulut_amd import _native, network      # noqa: E402
from mulut_amd.net_train import NetTrainer, step_flops, torch_predict      # noqa: E402

PEAK_F32_MFMA = 157.3e12
NF, SCALE, MODES, STAGES, CROP = 64, 4, "sdy", 2, 48


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def compare(variants, rounds):
    live = dict(variants)
    for k, fn in list(live.items()):
        try:
            fn()
            fn()
        except torch.cuda.OutOfMemoryError:
            del live[k]
            torch.cuda.empty_cache()
    torch.cuda.synchronize()
    times = {k: [] for k in live}
    for _ in range(rounds):
        for k, fn in live.items():
            times[k].append(timed(fn))
    out = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "times_ms": [round(t, 4) for t in v]} for k, v in times.items()}
    out.update({k: "out of device memory" for k in variants if k not in live})
    return out


def make_step(base, batch, path, ws_sites=None):
    model = copy.deepcopy(base).cuda()
    optim = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    trainer = None if path == "torch" else (NetTrainer(model) if ws_sites is None else NetTrainer(model, ws_sites=ws_sites))
    gen = torch.Generator(device="cuda").manual_seed(batch)
    im = torch.randint(0, 256, (batch, 1, CROP, CROP), device="cuda", generator=gen).float() / 255.0
    lb = torch.randint(0, 256, (batch, 1, CROP * SCALE, CROP * SCALE), device="cuda", generator=gen).float() / 255.0

    def step():
        optim.zero_grad()
        pred = torch_predict(model, im, MODES, STAGES, "train") if trainer is None else trainer.predict(im, "train")
        loss = F.mse_loss(pred, lb)
        loss.backward()
        optim.step()
        return loss
    step.trainer = trainer
    return step


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", default="8,32,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_train_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("net_train_bench.py: no GPU visible; nothing is measured without one")
    torch.manual_seed(0)
    base = network.SRNets(nf=NF, scale=SCALE, modes=list(MODES), stages=STAGES)
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _native.source_hash(), "rounds": args.rounds,
              "model": "seeded: nf %d, %s, x%d, %d stages; crop %d" % (NF, MODES, SCALE, STAGES, CROP), "peak_f32_mfma_tflops": PEAK_F32_MFMA / 1e12, "cases": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        variants = {"fused": make_step(base, batch, "fused"), "torch": make_step(base, batch, "torch")}
        variants["fused_one_chunk"] = make_step(base, batch, "fused", ws_sites=batch * CROP * CROP)
        first = {k: float(fn().detach()) for k, fn in variants.items() if k != "torch" or batch <= 32}
        r = compare(variants, args.rounds)
        flops = step_flops(NF, SCALE, MODES, STAGES, batch, CROP)
        case = {"batch": batch, "step_flops": flops, "first_loss": first, "variants": r, "sites_per_stage": batch * CROP * CROP,
                "workspace_bytes": {k: int(fn.trainer._ws.numel()) for k, fn in variants.items() if fn.trainer is not None},
                "chunk_sites": {k: min(fn.trainer.ws_sites, batch * CROP * CROP) for k, fn in variants.items() if fn.trainer is not None}}
        f, t = r["fused"], r["torch"]
        case["fused_tflops"] = flops / f["median_ms"] / 1e9
        case["fused_share_of_peak"] = case["fused_tflops"] / (PEAK_F32_MFMA / 1e12)
        if isinstance(t, dict):
            case["torch_over_fused"] = t["median_ms"] / f["median_ms"]
            case["gap_exceeds_spread_of_either"] = abs(t["median_ms"] - f["median_ms"]) > max(t["max_ms"] - t["min_ms"], f["max_ms"] - f["min_ms"])
        if isinstance(r.get("fused_one_chunk"), dict):
            o = r["fused_one_chunk"]
            case["one_chunk_over_default"] = o["median_ms"] / f["median_ms"]
            case["one_chunk_gap_exceeds_spread_of_either"] = abs(o["median_ms"] - f["median_ms"]) > max(o["max_ms"] - o["min_ms"], f["max_ms"] - f["min_ms"])
        result["cases"]["batch_%d" % batch] = case
        print(json.dumps({k: v for k, v in case.items() if k != "variants"}, default=str), {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in r.items()}, flush=True)
        del variants
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
