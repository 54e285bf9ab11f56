#!/usr/bin/env python3
"""Golden data for the fused network forward (mulut_net_*), made by RUNNING THE REFERENCE's own `mulut_predict` / `round_func`
(sr/1_train_model.py:26-55) over its `SRNets` (sr/model.py + common/network.py) on the CPU in this container -- same rules as
gen_golden_transfer.py.  Only data is written.

    python tests/golden/gen_golden_net.py      # rewrites tests/golden/net_fixtures.npz and its shards net_fixtures_pass<k>.npz

The modules the script imports but these functions do not need (cv2, tensorboard, sr/data.py) are stubbed.  `round_func` is wrapped by
a recorder that calls the reference's and keeps what it returns: per stage the twelve (M x 4) per-pass arrays in the order of the
script's loops (mode outer, rotation inner), then the stage's own rounding.

Models: `shipped` = models/sr_x2sdy/Model_200000.pth (2 stages, sdy, x4, nf 64); `tiny` = the seeded nf 8, 1 stage, x2 model whose
weights transfer_fixtures.npz holds as `tinyw/*` (rebuilt from the same seed, and checked against them).
Inputs: crops of the Set5 LR images of tests/golden/Set5/LR_bicubic/X4 at the smallest shapes at which a site-tiled kernel can go
wrong (1x1, 1x9, 9x1, 5x7, one past a 32 / 64 site tile each way, C 1 and 3, N 2).

Per case `<model>/<case>/`: `x` uint8 [N, C, H, W]; per stage s `s<s>/pass` int8 [12, N, C, H u, W u] and `s<s>/out` uint8 (the
stage's bytes: the next stage's input, or the result as sr/1_train_model.py:101 makes it); `f64_share` = [bytes of the result on
which the same procedure in float64 gives another byte, bytes], for information.
`set5/<name>/psnr`: the reference's Y-PSNR (common/utils.py PSNR, _rgb2ycbcr, shave = scale) of its own result on the whole image,
`set5/<name>/sha256` of those bytes (HWC), and `set5/train_log_psnr` = the 'AVG Val PSNR' of Set5 at iteration 200000 in the shipped
train.log.
"""
import copy
import hashlib
import importlib.util
import os
import re
import sys
import types

import numpy as np
import torch
from PIL import Image

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SET5 = ("baby", "bird", "butterfly", "head", "woman")

# name, image, (top, left), (H, W), C, N  (image n of a batch is the crop moved 7 px right and 3 px down)
CASES = {
    "shipped": [("1x1", "bird", (20, 30), (1, 1), 3, 1), ("1x9", "head", (11, 5), (1, 9), 1, 1), ("9x1", "woman", (40, 20), (9, 1), 3, 1),
                ("5x7", "butterfly", (30, 22), (5, 7), 3, 2), ("33x65", "baby", (40, 31), (33, 65), 1, 1),
                ("65x33", "bird", (2, 17), (65, 33), 1, 1), ("24x40", "butterfly", (17, 9), (24, 40), 3, 1)],
    "tiny": [("1x1", "bird", (20, 30), (1, 1), 3, 1), ("1x9", "head", (11, 5), (1, 9), 1, 1), ("9x1", "woman", (40, 20), (9, 1), 3, 1),
             ("5x7", "butterfly", (30, 22), (5, 7), 3, 2), ("33x65", "baby", (40, 31), (33, 65), 3, 2),
             ("65x33", "bird", (2, 5), (65, 33), 3, 2)],
}


def crop(name, top, left, H, W, C, N):
    im = np.array(Image.open(os.path.join(HERE, "Set5", "LR_bicubic", "X4", name + ".png")))
    out = np.stack([im[top + 3 * n:top + 3 * n + H, left + 7 * n:left + 7 * n + W, :C].transpose(2, 0, 1) for n in range(N)])
    assert out.shape == (N, C, H, W), (name, out.shape)
    return np.ascontiguousarray(out)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("gen_golden_net.py: /root/reference not present")
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    data = types.ModuleType("data")
    data.Provider = data.SRBenchmark = object
    sys.modules.setdefault("data", data)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "sr"))
    os.chdir(os.path.join(REF, "sr"))
    spec = importlib.util.spec_from_file_location("ref_train", os.path.join(REF, "sr", "1_train_model.py"))
    ref_train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_train)                          # __main__ guard keeps the script body from running
    import model as ref_model
    from common.utils import PSNR, _rgb2ycbcr

    recorded = []
    ref_round = ref_train.round_func

    def recorder(t):
        out = ref_round(t)
        recorded.append(out.detach().clone())
        return out
    ref_train.round_func = recorder

    def predict(net, x_u8, opt, dtype=torch.float32):
        """sr/1_train_model.py:93-101 on uint8 [N, C, H, W]: (bytes, per stage (pass [12, ...] int8, out uint8))."""
        del recorded[:]
        M = len(opt.modes)
        with torch.no_grad():
            x = torch.from_numpy(x_u8.astype(np.float32) / 255.0).to(dtype)
            pred = ref_train.mulut_predict(net, x, "valid", opt)
        res = np.round(np.clip(pred.numpy(), 0, 255)).astype(np.uint8)
        assert len(recorded) == opt.stages * (4 * M + 1)
        stages = []
        for s in range(opt.stages):
            rec = recorded[s * (4 * M + 1):(s + 1) * (4 * M + 1)]
            p = torch.stack(rec[:4 * M]).numpy()
            assert np.abs(p).max() <= 127 and np.array_equal(p, np.round(p))
            out = res if s + 1 == opt.stages else rec[4 * M].numpy()
            assert np.array_equal(out, np.round(out)) and out.min() >= 0 and out.max() <= 255
            stages.append((p.astype(np.int8), out.astype(np.uint8)))
        return res, stages

    fx = {}
    lm = torch.load(os.path.join(REF, "models", "sr_x2sdy", "Model_200000.pth"), map_location="cpu", weights_only=False)
    shipped = ref_model.SRNets(nf=64, scale=4, modes=list("sdy"), stages=2)
    shipped.load_state_dict(lm.state_dict(), strict=True)
    torch.manual_seed(11)
    tiny = ref_model.SRNets(nf=8, scale=2, modes=list("sdy"), stages=1)
    have = np.load(os.path.join(HERE, "transfer_fixtures.npz"))
    for k, v in tiny.state_dict().items():
        assert np.array_equal(have["tinyw/" + k], v.numpy()), k
    models = {"shipped": (shipped.eval(), types.SimpleNamespace(modes=list("sdy"), stages=2, scale=4)),
              "tiny": (tiny.eval(), types.SimpleNamespace(modes=list("sdy"), stages=1, scale=2))}
    for mname, (net, opt) in models.items():
        net64 = copy.deepcopy(net).double()
        total = 0
        for cname, img, (top, left), (H, W), C, N in CASES[mname]:
            x = crop(img, top, left, H, W, C, N)
            key = "%s/%s" % (mname, cname)
            res, stages = predict(net, x, opt)
            fx[key + "/x"] = x
            for s, (p, out) in enumerate(stages):
                fx["%s/s%d/pass" % (key, s + 1)] = p
                fx["%s/s%d/out" % (key, s + 1)] = out
                total += out.size
            res64, _ = predict(net64, x, opt, torch.float64)
            fx[key + "/f64_share"] = np.array([int((res64 != res).sum()), res.size], dtype=np.int64)
            print(key, x.shape, "->", res.shape, "f64 differs on", fx[key + "/f64_share"])
        print(mname, "output bytes", total)
        assert total >= 100000
    net, opt = models["shipped"]
    psnrs = []
    for name in SET5:
        lr = np.array(Image.open(os.path.join(HERE, "Set5", "LR_bicubic", "X4", name + ".png")))
        hr = np.array(Image.open(os.path.join(HERE, "Set5", "HR", name + ".png")))
        res, _ = predict(net, np.ascontiguousarray(lr.transpose(2, 0, 1)[None]), opt)
        pred = np.ascontiguousarray(res[0].transpose(1, 2, 0))
        hr = hr[:pred.shape[0], :pred.shape[1]]
        p = PSNR(_rgb2ycbcr(pred)[:, :, 0], _rgb2ycbcr(hr)[:, :, 0], opt.scale)      # :103-104
        fx["set5/%s/psnr" % name] = np.float64(p)
        fx["set5/%s/sha256" % name] = np.frombuffer(hashlib.sha256(pred.tobytes()).digest(), dtype=np.uint8)
        psnrs.append(p)
        print(name, pred.shape, p)
    log = open(os.path.join(REF, "models", "sr_x2sdy", "train.log")).read()
    fx["set5/train_log_psnr"] = np.float64(re.findall(r"Iter 200000 \| Dataset Set5 \| AVG Val PSNR: ([0-9.]+)", log)[-1])
    print("Set5 mean", np.mean(np.asarray(psnrs)), "train.log", fx["set5/train_log_psnr"])
    # The per-pass arrays are twelve values per output byte and do not compress (the passes of a stage are large and cancel).  No file
    # of the repository may exceed 1 MiB, so the arrays of 100,000 values and more go to shards net_fixtures_pass<k>.npz, first fit by
    # their deflated size into 900 KB; everything else is net_fixtures.npz.  tests/net_cases.py reads them back as one dictionary.
    import zlib
    shards, main = [], {}
    for k, v in fx.items():
        if not (k.endswith("/pass") and v.size >= 100000):
            main[k] = v
            continue
        z = len(zlib.compress(v.tobytes(), 6))
        for sh in shards:
            if sh["z"] + z <= 900000:
                break
        else:
            sh = {"z": 0, "fx": {}}
            shards.append(sh)
        sh["fx"][k] = v
        sh["z"] += z
    for old in os.listdir(HERE):
        if re.match(r"net_fixtures(_pass\d+)?\.npz$", old):
            os.remove(os.path.join(HERE, old))
    for name, d in [("net_fixtures.npz", main)] + [("net_fixtures_pass%d.npz" % k, sh["fx"]) for k, sh in enumerate(shards)]:
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **d)
        print(path, os.path.getsize(path), "bytes", len(d), "arrays")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
