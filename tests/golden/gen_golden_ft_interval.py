#!/usr/bin/env python3
"""Golden fixtures for LUT fine-tuning at the sampling intervals 5 and 6, produced by RUNNING THE REFERENCE's `MuLUT`
module (sr/model.py:39-312, constructed with interval = 5 / 6) on the CPU in the authoring container: forward output, loss,
input gradient and every parameter gradient of an MSE loss for a few seeded batches.  Only data is written
(tests/golden/ft_interval_fixtures.npz); the tables are rebuilt by the tests from seeds or read from interval_fixtures.npz.
Inert when /root/reference is absent.   python tests/golden/gen_golden_ft_interval.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
    # name, interval, stages, modes, scale, table source, input kind, shape
    ("A5_s2sdy_x4_u8", 5, 2, "sdy", 4, "transferred", "u8", (2, 1, 12, 10)),
    ("A6_s2sdy_x4_u8", 6, 2, "sdy", 4, "transferred", "u8", (2, 1, 12, 10)),
    ("C5_s2sd_x2_u8", 5, 2, "sd", 2, "synth", "u8", (3, 1, 8, 8)),
    ("B6_s1s_x3_float", 6, 1, "s", 3, "synth", "float", (1, 2, 7, 9)),
    ("E5_s3y_x1_grid", 5, 3, "y", 1, "synth", "grid", (1, 1, 9, 9)),
]


def synthetic_lut(interval, stage, mode, vnum):
    """Seeded int8 table with values -128..127 (-128 clamps to -127 in the module's quantiser: its backward mask)."""
    rng = np.random.default_rng(1000 * interval + 17 * stage + ord(mode))
    return rng.integers(-128, 128, size=((2 ** (8 - interval) + 1) ** 4, vnum), dtype=np.int8)


def case_tables(interval, stages, modes, scale, src):
    iv_fx = np.load(os.path.join(HERE, "interval_fixtures.npz")) if src == "transferred" else None
    out = {}
    for s in range(stages):
        vnum = scale * scale if s + 1 == stages else 1
        for m in modes:
            key = "s%d_%s" % (s + 1, m)
            t = iv_fx["iv%d/lut/%s" % (interval, key)] if iv_fx is not None else synthetic_lut(interval, s + 1, m, vnum)
            out[key] = np.ascontiguousarray(t.reshape(-1, vnum).astype(np.int8))
    return out


def case_input(name, kind, shape, interval):
    rng = np.random.default_rng(sum(map(ord, name)))
    if kind == "u8":
        x = rng.integers(0, 256, shape).astype(np.float32) / np.float32(255.0)
    elif kind == "grid":      # ties and both ends of the grid
        q = 2 ** interval
        x = rng.choice(np.array([0, q - 1, q, 256 - q, 255], np.float32), shape) / np.float32(255.0)
    else:
        x = rng.random(shape, dtype=np.float32)
    return x, rng


def main():
    if not os.path.isdir(REF):
        raise SystemExit("gen_golden_ft_interval.py: /root/reference not present")
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "sr"))
    cwd = os.getcwd()
    os.chdir(os.path.join(REF, "sr"))          # model.py does sys.path.insert(0, "../")
    try:
        import model as ref_model               # noqa: E402  (the reference's sr/model.py)
    finally:
        os.chdir(cwd)
    out = {}
    for name, interval, stages, modes, scale, src, kind, shape in CASES:
        luts = case_tables(interval, stages, modes, scale, src)
        with tempfile.TemporaryDirectory() as td:
            for key, t in luts.items():
                np.save(os.path.join(td, "LUT_x%d_%dbit_int8_%s.npy" % (scale, interval, key)), t)
            net = ref_model.MuLUT(td, stages, list(modes), upscale=scale, interval=interval)
        x, rng = case_input(name, kind, shape, interval)
        tgt = rng.random((shape[0], shape[1], shape[2] * scale, shape[3] * scale), dtype=np.float32)
        xt = torch.from_numpy(x).requires_grad_(True)
        y = net(xt)
        loss = torch.nn.functional.mse_loss(y, torch.from_numpy(tgt))
        loss.backward()
        out[name + "/x"] = x
        out[name + "/target"] = tgt
        out[name + "/y"] = y.detach().numpy()
        out[name + "/loss"] = np.float32(loss.item())
        out[name + "/grad_x"] = xt.grad.numpy()
        out[name + "/cfg"] = np.array([interval, stages, scale], dtype=np.int32)
        out[name + "/modes"] = np.frombuffer(modes.encode(), dtype=np.uint8)
        out[name + "/lutsrc"] = np.frombuffer(src.encode(), dtype=np.uint8)
        touched = {}
        for key in luts:
            g = getattr(net, "weight_" + key).grad.numpy()
            rows = np.nonzero(np.abs(g).sum(1))[0]
            out[name + "/grad/" + key + "/rows"] = rows.astype(np.int32)
            out[name + "/grad/" + key + "/vals"] = g[rows]
            touched[key] = len(rows)
        print(name, "loss %.6f" % loss.item(), "y", tuple(y.shape), touched)
    path = os.path.join(HERE, "ft_interval_fixtures.npz")
    np.savez_compressed(path, **out)
    print("wrote ft_interval_fixtures.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
