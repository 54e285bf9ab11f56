#!/usr/bin/env python3
"""In-tube statistics of the final stage's input per routing granularity.  CPU only (the oracle computes
the first stage): for one LR 1080x1920x3 frame of a distribution, the share of the 12 passes of a sample that stay in the tube
(max - min of the four MSBs <= 1), the share of samples with every pass in the tube ("clean"), and how both distribute over the
64x16 verdict tiles and over the 16x4 tiles a stage_tube2_kernel wave owns.
    python tools/tube_histogram.py [--dist real] [--h 1080 --w 1920] > profiles/r04_tube_histogram_real.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mulut_amd import load_lut_dict  # noqa: E402
from mulut_amd.synth import natural_frames, noise_frames, real_frames  # noqa: E402
from oracle import c_oracle  # noqa: E402

PAT = {"s": [(0, 1), (1, 0), (1, 1)], "d": [(0, 2), (2, 0), (2, 2)], "y": [(1, 1), (1, 2), (2, 1)]}


def rot(r, di, dj):
    return [(di, dj), (dj, -di), (-di, -dj), (-dj, di)][r]


def shifted(h, dy, dx):
    H, W = h.shape[:2]
    ys = np.clip(np.arange(H) + dy, 0, H - 1)
    xs = np.clip(np.arange(W) + dx, 0, W - 1)
    return h[ys][:, xs]


def flat_share(h, left, right, tw=16, th=4, halo=2):
    """Share of (tile, channel) pairs with max - min <= 1 over rows y0 - halo .. y0 + th + halo - 1, columns x0 - left .. x0 + right - 1 (clamped)."""
    H, W, C = h.shape
    flat = total = 0
    for y0 in range(0, H, th):
        rows = h[np.clip(np.arange(y0 - halo, y0 + th + halo), 0, H - 1)]
        for x0 in range(0, W, tw):
            blk = rows[:, np.clip(np.arange(x0 - left, x0 + right), 0, W - 1)]
            flat += int(((blk.max((0, 1)) - blk.min((0, 1))) <= 1).sum())
            total += C
    return round(flat / total, 5)


def fix2_skip_share(x):
    """Of the samples of x (uint8 HWC) the tube kernels list (a pass whose four key MSBs span more than one step), how many have all
    twelve passes within 32 levels in their pixel VALUES (mulut_core.h fix2_pass_far): stage_up_fix2_kernel leaves those alone.  Same
    clamps as the kernels on a whole frame: rows and columns replicated at the frame's edges."""
    v, h = x.astype(np.int16), (x >> 4).astype(np.int16)
    flagged, far = np.zeros(x.shape, bool), np.zeros(x.shape, bool)
    for m in "sdy":
        for r in range(4):
            offs = [rot(r, di, dj) for di, dj in PAT[m]]
            hs, vs = [h] + [shifted(h, *o) for o in offs], [v] + [shifted(v, *o) for o in offs]
            flagged |= (np.maximum.reduce(hs) - np.minimum.reduce(hs)) > 1
            far |= (np.maximum.reduce(vs) - np.minimum.reduce(vs)) > 32
    return {"samples": int(x.size), "flagged": int(flagged.sum()), "flagged_and_skippable": int((flagged & ~far).sum()),
            "far_but_not_flagged": int((far & ~flagged).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dist", default="real")
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--stage", type=int, default=2, help="2: statistics of the final stage's input (= first-stage output); 1: of the first stage's input")
    ap.add_argument("--skip-draws", type=int, default=0, help="K > 0: only the fix-up kernel's skippable share of the final stage's input, over draws 0 .. K - 1")
    a = ap.parse_args()
    png = os.path.join(ROOT, "tests", "golden", "DIV2K_LR_X4", "0001x4.png")
    frames = {"real": lambda n: real_frames(n, a.h, a.w, png, 0), "natural": lambda n: natural_frames(n, a.h, a.w, 3, 0),
              "noise": lambda n: noise_frames(n, a.h, a.w, 3, 0)}[a.dist]
    luts = load_lut_dict(os.path.join(ROOT, "tests", "golden", "luts"), 2, "sdy", 4, 4, "LUT_ft")
    if a.skip_draws > 0:
        per = [fix2_skip_share(c_oracle.stage([luts["s1_%s" % m] for m in "sdy"], "sdy", False, f, 1)) for f in frames(a.skip_draws)]
        tot = {k: sum(p[k] for p in per) for k in per[0]}
        print(json.dumps({"dist": a.dist, "stage_input": 2, "frame": [a.h, a.w, 3], "draws": a.skip_draws,
                          "rule": "flagged: a pass with key MSBs spanning more than one step; skippable: every pass within 32 levels",
                          "flagged_share_of_samples": round(tot["flagged"] / tot["samples"], 5),
                          "skippable_share_of_flagged": round(tot["flagged_and_skippable"] / max(tot["flagged"], 1), 5),
                          "total": tot, "per_draw": per}, indent=1))
        return
    img = frames(1)[0]
    x = img if a.stage == 1 else c_oracle.stage([luts["s1_%s" % m] for m in "sdy"], "sdy", False, img, 1)
    h = (x >> 4).astype(np.int8)        # HWC MSBs
    H, W, C = h.shape
    out_cnt = np.zeros((H, W, C), np.int16)      # passes of the sample that leave the tube
    for m in "sdy":
        for r in range(4):
            hs = [h] + [shifted(h, *rot(r, di, dj)) for di, dj in PAT[m]]
            mx = np.maximum(np.maximum(hs[0], hs[1]), np.maximum(hs[2], hs[3]))
            mn = np.minimum(np.minimum(hs[0], hs[1]), np.minimum(hs[2], hs[3]))
            out_cnt += (mx - mn > 1)
    dirty = out_cnt > 0
    rec = {"dist": a.dist, "stage_input": a.stage, "frame": [H, W, C], "passes_in_tube": round(1 - out_cnt.sum() / (12.0 * H * W * C), 5),
           "samples_clean": round(1 - dirty.mean(), 5),
           # share of the (16x4 wave tile, channel) pairs whose MSBs span at most one step: over the pixels the tile's windows read, and over
           # the whole 24x8 image of aligned dwords a stage_tube2_kernel wave stashes (the predicate it skips its tube tests on)
           "flat_tile_share_windows": flat_share(h, 2, 18), "flat_tile_share_stash_image": flat_share(h, 4, 20), "tiles": {}}
    for name, (tw, th) in (("64x16", (64, 16)), ("16x4", (16, 4)), ("16x16", (16, 16)), ("64x64", (64, 64))):
        Hp, Wp = -(-H // th) * th, -(-W // tw) * tw
        d = np.zeros((Hp, Wp, C), np.float64); d[:H, :W] = dirty
        v = np.zeros((Hp, Wp, C), np.float64); v[:H, :W] = 1
        o = np.zeros((Hp, Wp, C), np.float64); o[:H, :W] = out_cnt
        red = lambda z: z.reshape(Hp // th, th, Wp // tw, tw, C).sum((1, 3, 4))      # noqa: E731
        nd, nv, no = red(d), red(v), red(o)
        share = nd / nv                        # dirty-sample share per tile
        edges = [0, 1e-9, 0.01, 0.02, 0.05, 0.125, 0.25, 0.5, 0.75, 1.0000001]
        hist = np.histogram(share, bins=edges, weights=nv)[0] / nv.sum()
        t = {"tiles": int(share.size), "dirty_share_bins": ["0", "(0,1%]", "(1,2%]", "(2,5%]", "(5,12.5%]", "(12.5,25%]", "(25,50%]", "(50,75%]", "(75,100%]"],
             "samples_in_tiles_by_dirty_share": [round(float(z), 4) for z in hist],
             "pass_in_tube_share_of_tiles_median": round(float(np.median(1 - no / (12 * nv))), 4), "routing": []}
        for thr in (0.02, 0.05, 0.125, 0.25, 0.5):
            fast = share <= thr
            t["routing"].append({"tile_to_tube_kernel_if_dirty_share_le": thr, "samples_on_tube_kernel": round(float(nv[fast].sum() / nv.sum()), 4),
                                 "of_all_samples_on_fixup_list": round(float(nd[fast].sum() / nv.sum()), 5),
                                 "samples_on_slab_path": round(float(nv[~fast].sum() / nv.sum()), 4)})
        rec["tiles"][name] = t
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
