#!/usr/bin/env python3
"""Golden data for the 4 x 4 sampling patterns e, h, o (LUT transfer and inference), made by RUNNING THE REFERENCE's network code
(common/network.py SRNet / MuLUTUnit) on the CPU in this container -- same rules as gen_golden_transfer.py.

    python tests/golden/gen_golden_wide.py      # rewrites tests/golden/wide_fixtures.npz

The model: a seeded tiny cascade (nf = 8) with one unit per pattern E, H, O in each of two stages -- stage 1 at scale 1
(`Ex1`, `Hx1`, `Ox1`), stage 2 the final stage at scale 2.  The reference cannot construct `HxN` / `OxN` (common/network.py:185
compares the mode string with a list), so those two units are built as SRNet('Hx1') / SRNet('Ox1') with `.model` replaced by
MuLUTUnit('1x4', nf, upscale=2) and `.S = 2` -- exactly what the `HxN` / `OxN` branch would build.  `ExN` is constructed as is.

What is recorded (data only):
  * the weights (`tinyw/<state_dict key>`, keys `s{stage}_{mode}.model...` as the SRNets twin names them),
  * for each table: sha256 of the int8 table round(clamp(net(patch), -1, 1) * 127) over the full 17^4 grid (a slowest), its
    shape and 2048 sampled rows (indices in `idx`).  The network is fed 4 x 4 patches with a, b, c, d at its own taps,
  * per pattern and stage: a grid-aligned image (values in {0, 16, ..., 240}, `img/s{stage}_{mode}`) and the network's
    output on it, round(clamp(out, -1, 1) * 127) (`netout/s{stage}_{mode}`): every pass on such an image has weight 16 on a
    single table vertex, so LUT inference at rotation 0 equals 16 x this output at every interior site.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
TAPS = {"e": ((0, 0), (0, 3), (3, 0), (3, 3)), "h": ((0, 0), (2, 2), (2, 3), (3, 2)), "o": ((0, 0), (2, 2), (1, 3), (3, 1))}


def grid(interval):
    base = torch.arange(0, 257, 2 ** interval)
    base[-1] -= 1
    L = base.size(0)
    g = torch.cartesian_prod(base, base, base, base)            # a slowest ... d fastest (sr/2_transfer_to_lut.py:19-37)
    return g.reshape(-1, 4).float() / 255.0, L


def main():
    if not os.path.isdir(REF):
        raise SystemExit("gen_golden_wide.py: /root/reference not present")
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, REF)
    from common.network import MuLUTUnit, SRNet

    nf, scale = 8, 2
    torch.manual_seed(23)
    net = nn.Module()
    for stage, u in ((1, 1), (2, scale)):
        for mode in "eho":
            if u == 1:
                unit = SRNet("%sx1" % mode.upper(), nf=nf)
            elif mode == "e":
                unit = SRNet("ExN", nf=nf, upscale=u)
            else:
                unit = SRNet("%sx1" % mode.upper(), nf=nf)          # HxN / OxN: common/network.py:185 never matches
                unit.model = MuLUTUnit("1x4", nf, upscale=u)
                unit.S = u
            net.add_module("s%d_%s" % (stage, mode), unit)
    net.eval()

    fx = {}
    for k, v in net.state_dict().items():
        fx["tinyw/" + k] = v.numpy()
    x, L = grid(4)
    rng = np.random.default_rng(5)
    idx = np.sort(rng.choice(L ** 4, 2048, replace=False))
    fx["idx"] = idx
    with torch.no_grad():
        for stage in (1, 2):
            for mode in "eho":
                unit = getattr(net, "s%d_%s" % (stage, mode))
                patch = torch.zeros(x.shape[0], 1, 4, 4)
                for k, (i, j) in enumerate(TAPS[mode]):
                    patch[:, 0, i, j] = x[:, k]
                out = torch.cat([unit(patch[b:b + 8192]) for b in range(0, patch.shape[0], 8192)])
                q = torch.round(torch.clamp(out, -1, 1) * 127).numpy().astype(np.int8)      # sr/2_transfer_to_lut.py:108-109
                key = "tiny/s%d_%s" % (stage, mode)
                fx[key + "/sha256"] = np.frombuffer(hashlib.sha256(q.tobytes()).digest(), dtype=np.uint8)
                fx[key + "/shape"] = np.array(q.shape)
                fx[key + "/rows"] = q.reshape(q.shape[0], -1)[idx]
                img = (rng.integers(0, 16, (1, 1, 11, 13)) * 16).astype(np.uint8)
                y = unit(torch.from_numpy(img).float() / 255.0)
                fx["img/s%d_%s" % (stage, mode)] = img[0, 0]
                fx["netout/s%d_%s" % (stage, mode)] = torch.round(torch.clamp(y, -1, 1) * 127).numpy().astype(np.int8)[0, 0]
                print(key, q.shape, int(q.min()), int(q.max()), tuple(y.shape))
    np.savez_compressed(os.path.join(HERE, "wide_fixtures.npz"), **fx)


if __name__ == "__main__":
    main()
