#!/usr/bin/env python3
"""Golden data for training the network (mulut_net_stage_sum / mulut_net_stage_backward, mulut_amd.net_train), made by RUNNING THE
REFERENCE's own `mulut_predict(..., 'train')`, `F.mse_loss` and `.backward()` (sr/1_train_model.py:26-55,194-197) over its `SRNets` on
the CPU in this container -- same rules as gen_golden_net.py.  Only data is written.

    python tests/golden/gen_golden_net_train.py      # rewrites tests/golden/net_train_fixtures.npz

Models: `tiny` = the seeded nf 8, 1 stage, x2, sdy model whose weights transfer_fixtures.npz holds as `tinyw/*`; `sd2` = a seeded nf 8,
2 stages, x2, sd model (every bias drawn from U(-0.2, 0.2), as tests/net_cases.seeded_model does), its weights stored as `sd2w/*`.
Batches: [4, 1, 12, 12] and [2, 1, 5, 7] crops of the Set5 LR images of tests/golden/Set5/LR_bicubic/X4 (image n of a batch is the crop
moved 7 px right and 3 px down); the label is the block of the HR image of the output's size whose corner is the crop's corner x 4.

A case is kept only if (i) the reference's float32 and float64 runs give the same integers in every stage's pred and (ii) the smallest
|pre-activation| over layers 1-5 of every site of the batch is >= 1e-6 in float64 (tests/net_train_cases.min_preact): then no ReLU of
the float32 run can have taken another branch than the float64 run's, and the real g of the loss can be used as it is.  The first
candidate position of a list that passes is taken.

Per case `<model>/<case>/`: `x`, `lb` uint8 (the network sees them / 255 in float32); per stage `s<k>/sum` int16 = pred of
:30-35; `loss`, `loss64`; `grad/<parameter>` float32 and `grad64/<parameter>` float64 of every parameter; `min_preact`.
"""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SHAPES = {"4x12x12": (4, 12, 12), "2x5x7": (2, 5, 7)}
CANDIDATES = [(img, top, left) for img in ("bird", "butterfly", "baby", "head", "woman") for top, left in ((20, 30), (11, 5), (30, 22), (2, 17), (40, 20))]


def crops(name, top, left, N, H, W, u):
    lr = np.array(Image.open(os.path.join(HERE, "Set5", "LR_bicubic", "X4", name + ".png")))
    hr = np.array(Image.open(os.path.join(HERE, "Set5", "HR", name + ".png")))
    x = np.stack([lr[top + 3 * n:top + 3 * n + H, left + 7 * n:left + 7 * n + W, :1].transpose(2, 0, 1) for n in range(N)])
    lb = np.stack([hr[4 * (top + 3 * n):4 * (top + 3 * n) + H * u, 4 * (left + 7 * n):4 * (left + 7 * n) + W * u, :1].transpose(2, 0, 1) for n in range(N)])
    assert x.shape == (N, 1, H, W) and lb.shape == (N, 1, H * u, W * u), (name, x.shape, lb.shape)
    return np.ascontiguousarray(x), np.ascontiguousarray(lb)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("gen_golden_net_train.py: /root/reference not present")
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    data = types.ModuleType("data")
    data.Provider = data.SRBenchmark = object
    sys.modules.setdefault("data", data)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "sr"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    os.chdir(os.path.join(REF, "sr"))
    spec = importlib.util.spec_from_file_location("ref_train", os.path.join(REF, "sr", "1_train_model.py"))
    ref_train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_train)
    import model as ref_model
    import net_train_cases as tc
    from mulut_amd import network

    recorded = []
    ref_round = ref_train.round_func

    def recorder(t):
        out = ref_round(t)
        recorded.append(out.detach().clone())
        return out
    ref_train.round_func = recorder

    def run(net, x_u8, lb_u8, opt, dtype):
        """The reference's step on one batch: (per-stage pred sums, loss, {parameter: gradient})."""
        del recorded[:]
        M = len(opt.modes)
        net.zero_grad()
        x = torch.from_numpy(x_u8.astype(np.float32) / 255.0).to(dtype)
        lb = torch.from_numpy(lb_u8.astype(np.float32) / 255.0).to(dtype)
        loss = F.mse_loss(ref_train.mulut_predict(net, x, "train", opt), lb)
        loss.backward()
        assert len(recorded) == opt.stages * (4 * M + 1)
        sums = [torch.stack(recorded[s * (4 * M + 1):s * (4 * M + 1) + 4 * M]).sum(0).numpy() for s in range(opt.stages)]
        return sums, loss.item(), {k: p.grad.detach().clone().numpy() for k, p in net.named_parameters()}

    fx = {}
    torch.manual_seed(11)
    tiny = ref_model.SRNets(nf=8, scale=2, modes=list("sdy"), stages=1)
    have = np.load(os.path.join(HERE, "transfer_fixtures.npz"))
    for k, v in tiny.state_dict().items():
        assert np.array_equal(have["tinyw/" + k], v.numpy()), k
    torch.manual_seed(23)
    sd2 = ref_model.SRNets(nf=8, scale=2, modes=list("sd"), stages=2)
    with torch.no_grad():
        for p in sd2.parameters():
            if p.dim() == 1:
                p.uniform_(-0.2, 0.2)
    for k, v in sd2.state_dict().items():
        fx["sd2w/" + k] = v.numpy().copy()
    models = {"tiny": (tiny, types.SimpleNamespace(modes=list("sdy"), stages=1, scale=2)),
              "sd2": (sd2, types.SimpleNamespace(modes=list("sd"), stages=2, scale=2))}
    for mname, (net, opt) in models.items():
        net64 = copy.deepcopy(net).double()
        ours64 = network.SRNets(nf=8, scale=2, modes=opt.modes, stages=opt.stages).double()
        ours64.load_state_dict(net64.state_dict(), strict=True)
        for cname, (N, H, W) in SHAPES.items():
            for img, top, left in CANDIDATES:
                x, lb = crops(img, top, left, N, H, W, opt.scale)
                sums, loss, grads = run(net, x, lb, opt, torch.float32)
                sums64, loss64, grads64 = run(net64, x, lb, opt, torch.float64)
                same = all(np.array_equal(a, b) for a, b in zip(sums, sums64))
                # the smallest |pre-activation| of the batch, every stage on the float64 run's own input
                xs, mp = torch.from_numpy(x.astype(np.float32) / 255.0).double(), np.inf
                with torch.no_grad():
                    _, stage_sums = tc.predict_train(ours64, xs, opt.modes, opt.stages)
                for s in range(1, opt.stages + 1):
                    if s > 1:
                        xs = tc.round_func(torch.clamp(stage_sums[s - 2] / (len(opt.modes) * 4) + 127, 0, 255)) / 255.0
                    mp = min(mp, float(tc.min_preact(ours64, xs, opt.modes, s).min()))
                print(mname, cname, img, top, left, "same integers:", same, "min |pre-activation| %.3g" % mp)
                if same and mp >= 1e-6:
                    break
            else:
                raise SystemExit("no candidate passes for %s/%s" % (mname, cname))
            key = "%s/%s" % (mname, cname)
            fx[key + "/x"], fx[key + "/lb"] = x, lb
            for s, p in enumerate(sums):
                assert np.array_equal(p, np.round(p)) and np.abs(p).max() <= 127 * 4 * len(opt.modes)
                fx["%s/s%d/sum" % (key, s + 1)] = p.astype(np.int16)
            fx[key + "/loss"], fx[key + "/loss64"] = np.float32(loss), np.float64(loss64)
            fx[key + "/min_preact"] = np.float64(mp)
            for k in grads:
                fx["%s/grad/%s" % (key, k)] = grads[k].astype(np.float32)
                fx["%s/grad64/%s" % (key, k)] = grads64[k].astype(np.float64)
            print(key, "loss", loss, loss64)
    path = os.path.join(HERE, "net_train_fixtures.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes", len(fx), "arrays")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
