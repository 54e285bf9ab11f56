"""What the fine-tune driver defines once, without a GPU: the validation pair loader (mulut_amd/ft_val.py::iter_val_pairs) and its three
consumers, and the draw of a training sample (mulut_amd/ft_data.py::draw_sample) and its two."""
import argparse
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import crop_cases as CC
import val_cases as V


@pytest.fixture
def cuda_is_identity(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)


def test_one_loader_feeds_every_validation(tmp_path, monkeypatch, cuda_is_identity):
    """iter_val_pairs on the folder of val_cases.py (RGB pairs, a grey pair, an HR that is no multiple of the scale, stems with '_',
    three datasets that are not on disk): modcrop + replicate as computed here, in order; the shape test's text; and valid_steps,
    engine_valid_steps and DeviceValSet see no file but through it."""
    from mulut_amd import ft_val
    s = 4
    val, files = V.write_val_dir(tmp_path / "bench", s)
    opt = argparse.Namespace(valDir=val, valoutDir=str(tmp_path / "out"), scale=s, debug=False)      # B100, Urban100, Manga109: absent
    got = list(ft_val.iter_val_pairs(opt))
    assert [(ds, fn) for ds, fn, _, _ in got] == [(ds, fn) for ds in ("Set5", "Set14") for fn in files[ds]]
    assert ("Set14", "zz_grey.png") in [g[:2] for g in got] and ("Set5", "img_001.png") in [g[:2] for g in got]
    for ds, fn, lr, gt in got:
        hr = np.array(Image.open(os.path.join(val, ds, "HR", fn)))
        want_lr = np.array(Image.open(os.path.join(val, ds, "LR_bicubic", "X%d" % s, fn)))
        want_gt = hr[:hr.shape[0] - hr.shape[0] % s, :hr.shape[1] - hr.shape[1] % s]
        if fn == "zz_grey.png":
            assert want_gt.ndim == 2 and want_lr.ndim == 2
            want_gt, want_lr = np.stack([want_gt] * 3, 2), np.stack([want_lr] * 3, 2)
        if fn == "zz_odd.png":
            assert want_gt.shape[:2] == (hr.shape[0] - 2, hr.shape[1] - 3)
        for a, want in ((lr, want_lr), (gt, want_gt)):
            assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and a.flags["C_CONTIGUOUS"] and np.array_equal(a, want), (ds, fn)
    # one LR row less: the loader's error, word for word, after the pairs in front of it
    lr_file = os.path.join(val, "Set14", "LR_bicubic", "X%d" % s, "zz_odd.png")
    short = np.array(Image.open(lr_file))[:-1]
    Image.fromarray(short).save(lr_file)
    it, seen = ft_val.iter_val_pairs(opt), []
    with pytest.raises(ValueError) as e:
        for pair in it:
            seen.append(pair[:2])
    assert seen == [g[:2] for g in got[:-1]]
    assert str(e.value) == "Set14/zz_odd.png: LR {} x scale {} is not the modcropped HR {}".format(short.shape, s, got[-1][3].shape)

    # the consumers: a loader that reads no file at all, over a valDir that does not exist
    rng, calls = np.random.default_rng(3), []
    fake = [("SetA", "x_01.png", 5, 6), ("SetA", "x_02.png", 4, 7), ("SetB", "plain.png", 6, 5)]
    fake = [(ds, fn, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h * s, w * s, 3), dtype=np.uint8)) for ds, fn, h, w in fake]

    def loader(o):
        calls.append(o)
        return iter(fake)
    monkeypatch.setattr(ft_val, "iter_val_pairs", loader)
    monkeypatch.setattr(ft_val, "eval_y", lambda gt, out, shave: (float(gt.shape[0]), 0.5))
    opt = argparse.Namespace(valDir=str(tmp_path / "nowhere"), valoutDir=str(tmp_path / "out2"), scale=s, debug=True)

    class Net(torch.nn.Module):
        def forward(self, x):
            return torch.nn.functional.interpolate(x, scale_factor=s, mode="nearest")

        def install_into(self, engine):
            engine.installed = True

    class Engine:
        device = torch.device("cpu")

        def pipeline(self, x):
            return x

        def eval_y(self, gt, out, shave):
            return float(gt.shape[1]), 0.25

    lines = []
    res = ft_val.valid_steps(Net(), opt, 3, lines.append)
    assert calls == [opt] and list(res) == ["SetA", "SetB"] and res["SetA"] == (18.0, 0.5) and len(lines) == 2
    assert opt.valResults["SetA"].tolist() == [[20.0, 0.5], [16.0, 0.5]]
    assert sorted(os.listdir(os.path.join(opt.valoutDir, "SetA"))) == ["01_lutft.png", "02_lutft.png"]
    assert np.array_equal(np.array(Image.open(os.path.join(opt.valoutDir, "SetB", "plain_lutft.png"))), np.kron(fake[2][2], np.ones((s, s, 1), np.uint8)))
    engine = Engine()
    res = ft_val.engine_valid_steps(Net(), engine, opt, 3, lines.append)
    assert calls == [opt, opt] and engine.installed and res["SetB"].tolist() == [[20.0, 0.25]] and len(lines) == 4
    # DeviceValSet: every pair has come through the loader before the first device allocation -- a limit of 0 bytes ends it there
    with pytest.raises(ft_val.ValidationSetTooLarge) as e:
        ft_val.DeviceValSet(opt, max_bytes=0)
    assert calls == [opt] * 3 and e.value.nbytes == sum(2 * gt.size + 5 * lr.size for _, _, lr, gt in fake)
    fake[1] = fake[1][:2] + (fake[1][2].astype(np.uint16), fake[1][3])
    with pytest.raises(ValueError) as e:
        ft_val.DeviceValSet(opt, max_bytes=0)
    assert str(e.value) == "SetA/x_02.png: not a pair of 8-bit images"


@pytest.mark.parametrize("seed", [0, 1, 20240229])
def test_one_draw_order_feeds_both_providers(tmp_path_factory, monkeypatch, cuda_is_identity, seed):
    """draw_sample consumes random.Random(seed) as the host provider always has -- its six calls restated here -- over 4 batches of 8,
    and both providers take their samples from it."""
    from mulut_amd import ft_data
    shapes, sz = [(57, 86, 3), (60, 59, 1), (64, 64, 3), (5, 9, 3)], 5
    rng, ref = random.Random(seed), random.Random(seed)
    for _ in range(4 * 8):
        n = ref.choice(list(range(len(shapes))))
        i = ref.randint(0, shapes[n][0] - sz)
        j = ref.randint(0, shapes[n][1] - sz)
        c = ref.randrange(shapes[n][2])
        flips = (ref.uniform(0, 1) < 0.5) + 2 * (ref.uniform(0, 1) < 0.5)
        k = ref.choice([0, 1, 2, 3])
        assert ft_data.draw_sample(rng, shapes, sz) == (n, i, j, c, flips, k)
    assert rng.getstate() == ref.getstate()

    train = CC.write_set(tmp_path_factory.mktemp("crops"), 2)
    host, dev = ft_data.CropProvider(train, 2, sz, 8, seed), ft_data.DeviceCropProvider(train, 2, sz, 8, seed)
    taken, fixed = [], [(1, 3, 2, 0, 3, 1), (4, 0, 7, 2, 0, 3)]

    def draw(rng, shapes, patch):
        taken.append((rng, [tuple(sh) for sh in shapes], patch))
        return fixed[len(taken) % 2]
    monkeypatch.setattr(ft_data, "draw_sample", draw)
    im, lb = host.next()
    want = [fixed[(k + 1) % 2] for k in range(8)]
    want_im, want_lb = CC.apply_draws(host.pairs, want, sz, 2)
    assert len(taken) == 8 and all(t == (host.rng, [p[0].shape for p in host.pairs], sz) for t in taken)
    assert np.array_equal(im.numpy(), want_im) and np.array_equal(lb.numpy(), want_lb)
    del taken[:]
    assert dev.draw().tolist() == [list(t) for t in want]
    assert len(taken) == 8 and all(t == (dev.rng, [p[0].shape for p in host.pairs], sz) for t in taken)
