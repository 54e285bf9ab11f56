#!/usr/bin/env python3
"""What `--deterministic` costs a training step of the SR network: forward, backward and Adam on the shipped configuration (nf 64,
2 stages, sdy, x4, crops 48 x 48) with the default backward (mulut_net_stage_backward: the input gradient added with float atomics)
and with the exact one (mulut_net_stage_backward_exact: tap gradients stored, then gathered per pixel in a fixed order).

    python tools/net_exact_bench.py [--rounds 7] [--batches 8,32,128] [--out profiles/net_exact_bench.json]

Both variants are `net_train.NetTrainer.predict` steps as tools/net_train_bench.py builds them: each has its own copy of the same seeded
model and its own `torch.optim.Adam`, on the same random batch [B, 1, 48, 48] with a [B, 1, 192, 192] label, in one process.  Each
round times every variant once, alternating, after a warm-up of each; a time is a host clock around one step that ends in a device
synchronise.  Reported per batch size: median, minimum and maximum per variant, the ratio of the medians, whether the gap exceeds the
spread (max - min) of either, the bytes of both workspaces, and the first loss of both (the same forward: equal).  The deterministic
step is also run twice more from a fresh copy of the model and the resulting parameters compared bit for bit.  There is no CPU path:
without a GPU this fails.
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
from mulut_amd.net_train import NetTrainer      # noqa: E402

NF, SCALE, MODES, STAGES, CROP = 64, 4, "sdy", 2, 48


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def make_step(base, batch, deterministic):
    model = copy.deepcopy(base).cuda()
    optim = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    trainer = NetTrainer(model, deterministic=deterministic)
    gen = torch.Generator(device="cuda").manual_seed(batch)
    im = torch.randint(0, 256, (batch, 1, CROP, CROP), device="cuda", generator=gen).float() / 255.0
    lb = torch.randint(0, 256, (batch, 1, CROP * SCALE, CROP * SCALE), device="cuda", generator=gen).float() / 255.0

    def step():
        optim.zero_grad()
        loss = F.mse_loss(trainer.predict(im, "train"), lb)
        loss.backward()
        optim.step()
        return loss
    step.trainer, step.model = trainer, model
    return step


def reproducible(base, batch, steps=3):
    """`steps` deterministic steps from two fresh copies of the model: are all parameters the same bits?"""
    ends = []
    for _ in range(2):
        step = make_step(base, batch, True)
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ends.append([p.detach().clone() for p in step.model.parameters()])
        step.trainer.close()
    return all(torch.equal(a, b) for a, b in zip(*ends))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", default="8,32,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_exact_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("net_exact_bench.py: no GPU visible; nothing is measured without one")
    torch.manual_seed(0)
    base = network.SRNets(nf=NF, scale=SCALE, modes=list(MODES), stages=STAGES)
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _native.source_hash(), "rounds": args.rounds,
              "command": "python tools/net_exact_bench.py --rounds %d --batches %s" % (args.rounds, args.batches),
              "model": "seeded: nf %d, %s, x%d, %d stages; crop %d" % (NF, MODES, SCALE, STAGES, CROP), "cases": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        variants = {"default": make_step(base, batch, False), "deterministic": make_step(base, batch, True)}
        first = {k: float(fn().detach()) for k, fn in variants.items()}
        for fn in variants.values():      # the warm-up: every shape of the timed window has run
            fn()
            fn()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn))
        r = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "times_ms": [round(t, 4) for t in v]} for k, v in times.items()}
        d, e = r["default"], r["deterministic"]
        case = {"batch": batch, "sites_per_stage": batch * CROP * CROP, "first_loss": first, "variants": r,
                "workspace_bytes": {k: int(fn.trainer._ws.numel()) for k, fn in variants.items()},
                "deterministic_over_default": e["median_ms"] / d["median_ms"],
                "gap_ms": e["median_ms"] - d["median_ms"],
                "gap_exceeds_spread_of_either": abs(e["median_ms"] - d["median_ms"]) > max(d["max_ms"] - d["min_ms"], e["max_ms"] - e["min_ms"]),
                "deterministic_steps_reproducible": reproducible(base, batch)}
        result["cases"]["batch_%d" % batch] = case
        print(json.dumps({k: v for k, v in case.items() if k != "variants"}), {k: v["median_ms"] for k, v in r.items()}, flush=True)
        for fn in variants.values():
            fn.trainer.close()
        del variants
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
