"""mulut_resample_run on the GPU (-m gpu): every byte equals Pillow's Image.resize(..., Image.BICUBIC) -- the case list of
tests/resample_cases.py in both layouts, sizes around the kernel's tile, batches, a captured graph, a side stream, a real frame's
size, make_lr on Set5, the fine-tune providers with --makeLR against a directory Pillow wrote, and the test script's baseline line."""
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import crop_cases as CC
import resample_cases as RC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both_layouts(a, out_h, out_w):
    """a: uint8 HW or HWC -> the HWC result and the NCHW result brought back to a's form."""
    from mulut_amd.resample import bicubic
    hwc = bicubic(dev(a), (out_h, out_w)).cpu().numpy()
    a3 = a if a.ndim == 3 else a[:, :, None]
    chw = bicubic(dev(a3.transpose(2, 0, 1)[None]), (out_h, out_w)).cpu().numpy()[0].transpose(1, 2, 0)
    return hwc, np.ascontiguousarray(chw if a.ndim == 3 else chw[:, :, 0])


def tile_cases():
    """(in_h, in_w, out_h, out_w): output widths at a tile's width (84 pixels of packed RGB, 256 of one channel), one below and one
    above; output heights at a tile's 16 rows (64 where the image grows) likewise; W % s and H % s take every residue."""
    from mulut_amd import resample
    tw3, tw1, th, thu = resample.tile_w(3), resample.tile_w(1), resample.TILE_H, resample.TILE_H_UP
    assert (tw3, tw1, th, thu) == (84, 256, 16, 64) and resample.tile_w(3, packed=False) == 256
    outs = list(zip([tw3 - 1, tw3, tw3 + 1, tw1 - 1, tw1, tw1 + 1], [th - 1, th, th + 1, thu - 1, thu, thu + 1]))
    cases, residues = [], {s: set() for s in RC.SCALES}
    for idx, (ow, oh) in enumerate(outs):
        for s in RC.SCALES:
            r = idx % s
            residues[s].add(r)
            cases.append((oh * s + (s - 1 - r), ow * s + r, oh, ow))
        for s in (2, 4):                                       # upscaling onto the same output sizes (ratios other than s too)
            cases.append(((oh + s - 1) // s, (ow + s - 1) // s, oh, ow))
    assert all(residues[s] == set(range(s)) for s in RC.SCALES)
    return cases


def test_case_list_in_both_layouts_equals_pillow():
    n = 0
    for h, w, kind, ch, oh, ow in RC.cases():
        a = RC.image(h, w, kind, ch)
        want = RC.pil_resize(a, oh, ow)
        for got in both_layouts(a, oh, ow):
            assert got.shape == want.shape and np.array_equal(got, want), (h, w, kind, ch, oh, ow)
        n += 1
    assert n >= 300


def test_sizes_around_the_tile_and_every_residue():
    for k, (h, w, oh, ow) in enumerate(tile_cases()):
        for ch in (3, 0):
            a = RC.image(h, w, ("ends", "noise")[k % 2], ch, seed=k)
            want = RC.pil_resize(a, oh, ow)
            for got in both_layouts(a, oh, ow):
                assert np.array_equal(got, want), (h, w, oh, ow, ch)


@pytest.mark.parametrize("h,w,oh,ow", [(37, 53, 37, 26), (37, 53, 18, 53), (48, 48, 48, 192), (48, 50, 192, 50), (20, 30, 20, 30)])
def test_an_unchanged_axis_is_skipped_as_pillow_skips_it(h, w, oh, ow):
    for kind in ("ends", "noise"):
        a = RC.image(h, w, kind, 3)
        want = RC.pil_resize(a, oh, ow)
        for got in both_layouts(a, oh, ow):
            assert np.array_equal(got, want)


@pytest.mark.parametrize("C", [2, 4, 5])
def test_any_channel_count_packed(C):
    """HWC with 2 and 4 channels (their own instances of the kernel) and 5 (one channel per workgroup, pixel stride 5): the channels
    are independent, so each equals Pillow on that channel alone."""
    from mulut_amd.resample import bicubic
    rng = np.random.default_rng(C)
    a = (rng.integers(0, 2, (70, 131, C), dtype=np.uint8) * 255)
    a[:35] = rng.integers(0, 256, (35, 131, C), dtype=np.uint8)
    for oh, ow in ((17, 32), (140, 262)):
        got = bicubic(dev(a), (oh, ow)).cpu().numpy()
        for c in range(C):
            assert np.array_equal(got[:, :, c], RC.pil_resize(np.ascontiguousarray(a[:, :, c]), oh, ow)), (C, c, oh, ow)


def test_a_batch_equals_single_calls():
    from mulut_amd.resample import bicubic
    frames = np.stack([RC.image(67, 131, kind, 3, seed=9) for kind in RC.CONTENTS])      # [3][67][131][3]
    x = dev(frames.transpose(0, 3, 1, 2))
    for oh, ow in ((33, 65), (22, 43), (134, 262)):
        got = bicubic(x, (oh, ow))
        assert got.shape == (3, 3, oh, ow)
        for i in range(3):
            assert torch.equal(got[i:i + 1], bicubic(x[i:i + 1], (oh, ow)))
            assert np.array_equal(got[i].cpu().numpy().transpose(1, 2, 0), RC.pil_resize(frames[i], oh, ow))


def test_a_large_batch_walks_several_tiles_per_workgroup():
    """200 planes of 70 x 301 -> 280 x 1204: 5 x 5 tiles of 64 rows x 256 pixels per plane, 5000 in the call, so a workgroup walks two
    tiles down its column and the last walker of a column one."""
    from mulut_amd.resample import bicubic
    planes = np.stack([RC.image(70, 301, kind, 0, seed=s) for s, kind in enumerate(("noise", "ends", "ramp", "noise"))])
    want = torch.from_numpy(np.stack([RC.pil_resize(p, 280, 1204) for p in planes])).cuda()
    got = bicubic(dev(planes)[None].expand(50, 4, 70, 301).contiguous(), (280, 1204))
    assert got.shape == (50, 4, 280, 1204) and bool((got == want[None]).all())


def test_graph_capture_and_replay_on_new_bytes():
    from mulut_amd.resample import bicubic
    frames = [RC.image(67, 131, kind, 3, seed=s) for s, kind in enumerate(RC.CONTENTS)]
    x, out = dev(frames[0]), torch.zeros((16, 32, 3), dtype=torch.uint8, device="cuda")
    bicubic(x, (16, 32), out=out)                 # the plan exists before the capture: a run allocates nothing and waits for nothing
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bicubic(x, (16, 32), out=out)
    for f in frames[1:]:
        x.copy_(torch.from_numpy(f))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), RC.pil_resize(f, 16, 32))


def test_a_run_on_a_side_stream_is_ordered_with_the_copy_behind_it():
    from mulut_amd.resample import bicubic
    a = RC.image(540, 960, "noise", 3)
    x = dev(a)
    bicubic(x, (270, 480))                        # (the plan: created on the null stream, with a blocking copy)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    host = torch.empty((270, 480, 3), dtype=torch.uint8).pin_memory()
    with torch.cuda.stream(side):
        y = bicubic(x, (270, 480))
        host.copy_(y, non_blocking=True)
    side.synchronize()
    assert np.array_equal(host.numpy(), RC.pil_resize(a, 270, 480))


def test_a_real_frames_size():
    from mulut_amd.resample import bicubic
    from mulut_amd.synth import natural_frames
    a = natural_frames(1, 1356, 2040, 3, seed=5)[0]
    assert np.array_equal(bicubic(dev(a), (339, 510)).cpu().numpy(), RC.pil_resize(a, 339, 510))


def test_make_lr_writes_pillows_bytes_in_both_layouts(tmp_path):
    from mulut_amd.resample import make_lr
    hr_dir = os.path.join(GOLDEN, "Set5", "HR")
    logs = []
    for layout, scales in (("div2k", (2, 3, 4)), ("benchmark", (4,))):
        root = str(tmp_path / layout)
        written = make_lr(hr_dir, root, scales, layout, log=logs.append)
        assert len(written) == 5 * len(scales)
        for fn in sorted(os.listdir(hr_dir)):
            img = Image.open(os.path.join(hr_dir, fn))
            for s in scales:
                path = os.path.join(root, "LR", "X%d" % s, "%sx%d.png" % (fn[:-4], s)) if layout == "div2k" else \
                    os.path.join(root, "LR_bicubic", "X%d" % s, fn)
                assert path in written
                got = Image.open(path)
                want = img.resize((img.width // s, img.height // s), resample=Image.BICUBIC)
                assert got.mode == want.mode and got.size == want.size and np.array_equal(np.array(got), np.array(want)), path
    assert not any("host" in ln for ln in logs)
    # a palette image takes Pillow on the host, and says so
    pal_dir = tmp_path / "pal" / "HR"
    pal_dir.mkdir(parents=True)
    pal = Image.fromarray(RC.image(40, 52, "noise", 3)).convert("P", palette=Image.ADAPTIVE, colors=16)
    pal.save(str(pal_dir / "p.png"))
    logs = []
    make_lr(str(pal_dir), str(tmp_path / "pal"), (2,), "benchmark", log=logs.append)
    assert sum("mode P" in ln and "host" in ln for ln in logs) == 1
    got = Image.open(str(tmp_path / "pal" / "LR_bicubic" / "X2" / "p.png"))
    want = Image.open(str(pal_dir / "p.png")).resize((26, 20), resample=Image.BICUBIC)
    assert got.mode == want.mode and np.array_equal(np.array(got), np.array(want))


@pytest.mark.parametrize("scale", [3, 4])
def test_finetune_batches_with_make_lr_equal_those_of_pillows_files(tmp_path, scale):
    """An HR-only copy of crop_cases' training directory with make_lr, against the same HR files beside LR files Pillow wrote on the
    host: the first 8 batches of either provider are bit-identical.  (d_ragged's HR sizes are no multiples of the scale.)"""
    from mulut_amd import finetune_lut
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider
    full = CC.write_set(tmp_path / "full", scale)
    hr_only, pillow = tmp_path / "hr_only", tmp_path / "pillow"
    for d in (hr_only, pillow):
        shutil.copytree(os.path.join(full, "HR"), str(d / "HR"))
    os.makedirs(str(pillow / "LR_bicubic" / ("X%d" % scale)))
    for fn in sorted(os.listdir(str(pillow / "HR"))):
        img = Image.open(str(pillow / "HR" / fn))
        img.resize((img.width // scale, img.height // scale), resample=Image.BICUBIC).save(str(pillow / "LR_bicubic" / ("X%d" % scale) / fn))
    for provider in (DeviceCropProvider, CropProvider):
        with pytest.raises(FileNotFoundError):
            provider(str(hr_only), scale, 48, 6, 11)
        made = provider(str(hr_only), scale, 48, 6, 11, make_lr=True)
        ref = provider(str(pillow), scale, 48, 6, 11)
        for k in range(8):
            (im, lb), (want_im, want_lb) = made.next(), ref.next()
            assert torch.equal(im, want_im) and torch.equal(lb, want_lb), (provider.__name__, k)
    assert finetune_lut.build_parser().parse_args(["-e", str(tmp_path)]).makeLR is False
    assert finetune_lut.build_parser().parse_args(["-e", str(tmp_path), "--makeLR"]).makeLR is True


@pytest.fixture(scope="module")
def set5(tmp_path_factory):
    """(the test script's arguments for Set5 with the shipped tables, float64 [5][2]: metrics.py on Pillow's x4 upscales of the LR files)"""
    from mulut_amd import metrics
    tmp_path = tmp_path_factory.mktemp("baseline")
    test_dir = tmp_path / "SRBenchmark"
    (test_dir / "Set5").mkdir(parents=True)
    os.symlink(os.path.join(GOLDEN, "Set5", "HR"), test_dir / "Set5" / "HR")
    os.symlink(os.path.join(GOLDEN, "Set5", "LR_bicubic"), test_dir / "Set5" / "LR_bicubic")
    exp = tmp_path / "models" / "sr_x2sdy"
    exp.mkdir(parents=True)
    for fn in os.listdir(os.path.join(GOLDEN, "luts")):
        os.symlink(os.path.join(GOLDEN, "luts", fn), exp / fn)
    argv = ["--stages", "2", "--modes", "sdy", "-e", str(exp), "--testDir", str(test_dir), "--resultRoot", str(tmp_path / "results")]
    want = []
    for fn in sorted(os.listdir(os.path.join(GOLDEN, "Set5", "HR"))):
        lr = Image.open(os.path.join(GOLDEN, "Set5", "LR_bicubic", "X4", fn))
        up = np.array(lr.resize((lr.width * 4, lr.height * 4), resample=Image.BICUBIC))
        gt = metrics.modcrop(np.array(Image.open(os.path.join(GOLDEN, "Set5", "HR", fn))), 4)
        y_gt, y_up = metrics.rgb2ycbcr(gt)[:, :, 0], metrics.rgb2ycbcr(up)[:, :, 0]
        want.append([metrics.psnr(y_gt, y_up, 4), metrics.ssim(y_gt, y_up)])
    return argv, np.asarray(want)


def baseline_line(want):
    return 'Dataset Set5 | AVG Bicubic PSNR: {:.2f} SSIM: {:.4f}'.format(np.mean(want[:, 0]), np.mean(want[:, 1]))


def test_test_script_baseline_line(set5, capsys):
    from mulut_amd import test_lut
    from mulut_amd.options import TestOptions
    argv, want = set5
    assert TestOptions().parse(argv).bicubicBaseline is False
    test_lut.main(argv)
    plain = capsys.readouterr().out
    assert plain.strip().splitlines()[-1].startswith("Dataset Set5 | AVG LUT PSNR: 30.61 SSIM: 0.865")
    opt = TestOptions().parse(argv + ["--bicubicBaseline"])
    e = test_lut.eltr("Set5", opt, test_lut.build_engine(opt))
    e.run()
    flagged = capsys.readouterr().out
    assert flagged.startswith(plain) and len(flagged.splitlines()) == len(plain.splitlines()) + 1
    assert np.array_equal(e.baseline, want)                                # as doubles
    assert flagged.splitlines()[-1] == baseline_line(want)
    test_lut.main(argv)                                                    # and an evaluator without the flag still prints no such line
    assert capsys.readouterr().out == plain


def test_test_script_baseline_line_from_the_command_line(set5):
    """python -m mulut_amd.test_lut: there the evaluator lives in __main__, and that is the class the flag has to reach."""
    import subprocess
    import sys
    from conftest import ROOT
    argv, want = set5
    r = subprocess.run([sys.executable, "-m", "mulut_amd.test_lut"] + argv + ["--bicubicBaseline"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2].startswith("Dataset Set5 | AVG LUT PSNR: 30.61 SSIM: 0.865") and lines[-1] == baseline_line(want)
