#!/usr/bin/env python3
"""Golden data for the sampling intervals 5 and 6, made by RUNNING THE REFERENCE in the authoring container (same rules as
gen_golden.py: it refuses to run without the reference, and writes data only).

    python tests/golden/gen_golden_interval.py      # rewrites tests/golden/interval_fixtures.npz

What is recorded, for interval 5 and 6 (prefix `iv5/`, `iv6/`):
  * `lut/s{stage}_{mode}`: the six tables the reference's transfer (sr/2_transfer_to_lut.py:80-116: its grid, its 100-chunk
    batching, round(clamp(net, -1, 1) * 127)) makes from the shipped checkpoint Model_200000.pth (2-stage sdy x4 SRNets), as
    int8 (L^4, v_num);
  * `pass/{input}/u{u}/{mode}/r{r}/sha256`: sha256 of q * FourSimplexInterpFaster (sr/4_test_lut.py:14-237) as the driver calls it
    (:289-298), as int32 C-order bytes, for the inputs of gen_golden.py's shapes plus extreme and tie inputs (`in/{input}`), modes
    s, d, y, all four rotations, u = 1 with the stage-1 table and u = 4 with the stage-2 table of that mode; `.../q` holds the array
    itself (int16: |q out| <= 128 q) when it has at most kArrayMax elements (the file stays under the size limit);
  * `crop/stage1`, `crop/final_sha256`: the reference's stage loop (:279-306) on a 64x64x3 crop of the shipped DIV2K LR image
    (`in/crop`): the stage-1 image, and sha256 of the final 256x256x3 one (uint8, C order);
  * `set5/{stem}/sha256`: sha256 of the HR pixels (uint8 H x W x 3, C order) the reference's eltr._worker (:261-310) writes for
    Set5 x4 with those tables, and `set5/summary`: the line eltr.run prints (:258).  Two reference quirks are worked around here
    (SURVEY.md): its LR path 'LR_bicubic/X'.format(scale) drops the scale (quirk 1), so the LR images are placed under that path;
    its reader wants {8-interval}bit file names while the writers write {interval}bit (quirk 3), so the tables are handed to it
    as the dict it would have loaded.
"""
import hashlib
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402  (the reference loader and the input recipes)

REF = gen_golden.REF
kArrayMax = 2048


def grid(interval):
    base = torch.arange(0, 257, 2 ** interval)
    base[-1] -= 1
    g = torch.cartesian_prod(base, base, base, base)            # a slowest ... d fastest, as :19-37
    return g.reshape(-1, 1, 2, 2).float() / 255.0


def transfer(net, ref_transfer, interval):
    """sr/2_transfer_to_lut.py:80-116 on the CPU (the reference builds the same grid with .cuda())."""
    out = {}
    net.eval()
    for s in range(2):
        for mode in "sdy":
            x = grid(interval)
            if mode != "s":
                x = ref_transfer.get_mode_input_tensor(x, mode)
            B = x.size(0) // 100
            parts = []
            with torch.no_grad():
                for b in range(100):
                    xb = x[b * B:] if b == 99 else x[b * B:(b + 1) * B]
                    parts.append(torch.round(torch.clamp(net(xb, stage=s + 1, mode=mode), -1, 1) * 127).numpy().astype(np.int8))
            t = np.concatenate(parts, 0)
            out["s%d_%s" % (s + 1, mode)] = t.reshape(t.shape[0], -1)
    return out


def ref_pass(t4, lut_f32, img_hwc_u8, r, u, mode, interval):
    img = img_hwc_u8.astype(np.float32)
    pad = (0, 2) if mode in "dy" else (0, 1)
    rimg = np.rot90(img, r)
    h, w, _ = rimg.shape
    img_in = np.pad(rimg, (pad, pad, (0, 0)), mode="edge").transpose((2, 0, 1))
    k = np.asarray(t4.FourSimplexInterpFaster(lut_f32, img_in, h, w, interval, 4 - r, upscale=u, mode=mode)) * 2.0 ** interval
    ki = np.rint(k).astype(np.int32)
    assert np.array_equal(ki.astype(np.float64), k), "reference pass is not a multiple of 1/q"
    assert np.abs(ki).max() <= 128 * 2 ** interval
    return ki


def ref_stages(t4, luts, img_hwc_u8, interval):
    """sr/4_test_lut.py:279-306 (2 stages, sdy, x4) around the reference's pass function."""
    img = img_hwc_u8.astype(np.float32)
    outs = []
    for s in range(2):
        last = s == 1
        upscale, avg, bias = (4, 3, 0) if last else (1, 12, 127)
        pred = 0
        for mode in "sdy":
            pad = (0, 2) if mode in "dy" else (0, 1)
            for r in range(4):
                rimg = np.rot90(img, r)
                h, w, _ = rimg.shape
                img_in = np.pad(rimg, (pad, pad, (0, 0)), mode="edge").transpose((2, 0, 1))
                pred = pred + t4.FourSimplexInterpFaster(luts["s%d_%s" % (s + 1, mode)], img_in, h, w, interval, 4 - r,
                                                         upscale=upscale, mode=mode)
        img = np.round(np.clip(np.clip(pred / avg + bias, 0, 255).transpose((1, 2, 0)), 0, 255))
        img = img.astype(np.uint8) if last else img.astype(np.float32)
        outs.append(img.astype(np.uint8))
    return outs


def ref_set5(t4, luts, interval):
    """eltr._worker for every Set5 image, run in-process (eltr.run only adds a Pool); it reads the globals `opt` and `dataset`."""
    from types import SimpleNamespace
    shas, ps = {}, []
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(REF, "data", "SRBenchmark", "Set5")
        os.makedirs(os.path.join(td, "Set5", "LR_bicubic"))
        os.symlink(os.path.join(src, "HR"), os.path.join(td, "Set5", "HR"))
        os.symlink(os.path.join(src, "LR_bicubic", "X4"), os.path.join(td, "Set5", "LR_bicubic", "X"))     # quirk 1
        opt = SimpleNamespace(stages=2, modes="sdy", scale=4, interval=interval, testDir=td, resultRoot=os.path.join(td, "res"),
                              expDir=os.path.join(td, "sr_iv"), lutName="LUT")
        t4.opt, t4.dataset = opt, "Set5"
        etr = t4.eltr("Set5", opt, {k: v.astype(np.float32) for k, v in luts.items()})
        for i, fn in enumerate(etr.files):
            ps.append(etr._worker(i))
            px = np.ascontiguousarray(np.array(Image.open(os.path.join(etr.result_path, "%s_LUT_%dbit.png" % (fn[:-4], 8 - interval)))))
            shas[fn[:-4]] = hashlib.sha256(px.tobytes()).hexdigest()
    ps = np.asarray(ps)
    return shas, "Dataset {} | AVG LUT PSNR: {:.2f} SSIM: {:.4f}".format("Set5", np.mean(ps[:, 0]), np.mean(ps[:, 1]))


def pass_inputs(interval):
    q = 2 ** interval
    rng = np.random.default_rng(4321 + interval)
    cases = {"rand_19x13x3": rng.integers(0, 256, (19, 13, 3), dtype=np.uint8),
             "rand_8x31x1": rng.integers(0, 256, (8, 31, 1), dtype=np.uint8),
             "rand_5x4x2": rng.integers(0, 256, (5, 4, 2), dtype=np.uint8),
             "one_1x1x1": np.array([[[200]]], dtype=np.uint8)}
    # ties: every pixel shares one LSB -> every comparison of the simplex sort is a tie
    cases["ties_6x5x3"] = (rng.integers(0, 256 // q, (6, 5, 3)) * q + q // 2 - 1).astype(np.uint8)
    # extremes: grid values, the top cell (MSB 255 >> interval: corner index L - 1), LSB 0 and q - 1
    ext = np.array([0, q - 1, q, 255 - q, 256 - q, 255], dtype=np.uint8)
    cases["extreme_5x6x3"] = ext[rng.integers(0, len(ext), (5, 6, 3))]
    return cases


def main():
    t4, _ = gen_golden._load_reference()
    sys.path.insert(0, os.path.join(REF, "sr"))
    cwd = os.getcwd()
    os.chdir(os.path.join(REF, "sr"))
    spec = importlib.util.spec_from_file_location("ref_transfer", os.path.join(REF, "sr", "2_transfer_to_lut.py"))
    ref_transfer = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_transfer)                       # __main__ guard keeps the script body from running
    import model as ref_model
    os.chdir(cwd)
    lm = torch.load(os.path.join(REF, "models", "sr_x2sdy", "Model_200000.pth"), map_location="cpu", weights_only=False)
    net = ref_model.SRNets(nf=64, scale=4, modes=list("sdy"), stages=2)
    net.load_state_dict(lm.state_dict(), strict=True)

    fx = {}
    crop = np.array(Image.open(os.path.join(REF, "data/DIV2K/LR/X4/0001x4.png")))[100:164, 200:264, :3]
    fx["in/crop"] = np.ascontiguousarray(crop)
    for iv in (5, 6):
        p = "iv%d/" % iv
        luts = transfer(net, ref_transfer, iv)
        for k, t in luts.items():
            fx[p + "lut/" + k] = t
            print(p + k, t.shape, t.min(), t.max())
        f32 = {k: v.astype(np.float32) for k, v in luts.items()}
        for name, img in pass_inputs(iv).items():
            fx[p + "in/" + name] = img
            for u, st in ((1, 1), (4, 2)):
                for m in "sdy":
                    for r in range(4):
                        k = ref_pass(t4, f32["s%d_%s" % (st, m)], img, r, u, m, iv)
                        key = p + "pass/%s/u%d/%s/r%d/" % (name, u, m, r)
                        fx[key + "sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(k, dtype=np.int32).tobytes()).hexdigest())
                        if k.size <= kArrayMax:
                            fx[key + "q"] = k.astype(np.int16)
        s1, fin = ref_stages(t4, f32, crop, iv)
        fx[p + "crop/stage1"] = s1
        fx[p + "crop/final_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(fin).tobytes()).hexdigest())
        shas, summary = ref_set5(t4, luts, iv)
        for stem, h in shas.items():
            fx[p + "set5/%s/sha256" % stem] = np.array(h)
        fx[p + "set5/summary"] = np.array(summary)
        print(p, summary)
    np.savez_compressed(os.path.join(HERE, "interval_fixtures.npz"), **fx)


if __name__ == "__main__":
    main()
