"""The fine-tune loop and its validation against the reference, one step at a time (-m gpu): mulut_amd/finetune_lut.py::FinetuneRun
and valid_steps, the twins of sr/3_finetune_lut.py:68-172 and :23-65.  The reference stepper, the cases and the bars are those of
tests/ft_loop_cases.py (what the cases reach is asserted on the reference alone in test_ft_loop_cpu.py).

Every step of every case starts from the state the device holds:
  forward     the bytes of the oracle -- x and the quantised tables are integers, so every float32 sum is exact (ft_exact_cases.py)
  loss        the oracle's float64 MSE within 4 x LOSS_F32_REL (what float32 costs F.mse_loss on the CPU, times 4 for the device's order)
  gradients   ft_grad_bar.close, and exactly zero beyond the quantiser's clamp
  optimiser   float64 Adam fed the device's own gradient; the device's Adam may be twice as far from it, in float32 ulps of each
              element, as torch's unfused float32 Adam on the CPU on the same inputs is (and 1 ulp at the least); no element left out.
              torch's fused=True misses that bar (measured: 234 ulps where the CPU is 60 off, 30.6 against 14.5, 8.5 against 0.86 -- and
              174 where the CPU is 430 off: the largest distance is that of ONE element that lands near zero, where every float32 Adam
              carries 1e-7 of the step); the driver's optimiser is mulut_amd.finetune.Adam, float64 arithmetic rounded once: 0.5 ulp
  schedule    the learning rate the step runs at is lr0 * lf(i - 1)
"""
import argparse
import os

import numpy as np
import pytest
from PIL import Image

import abi_sequences as A
import ft_loop_cases as L
from conftest import GOLDEN
from ft_grad_bar import close

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import finetune_lut  # noqa: E402


def make_run(case, tmp_path, host=True):
    train = L.write_pairs(tmp_path / "train", case.scale)
    exp = L.write_tables(case, tmp_path / "exp")
    lines = []
    opt = finetune_lut.build_parser().parse_args(
        ["--stages", str(case.stages), "--modes", case.modes, "--scale", str(case.scale), "--interval", str(case.interval), "-e", exp,
         "--trainDir", train, "--batchSize", str(case.batch), "--cropSize", str(case.crop), "--totalIter", str(case.K),
         "--displayStep", str(L.DISPLAY_STEP), "--valStep", "0", "--lr0", repr(case.lr0), "--lr1", repr(case.lr1),
         "--weightDecay", repr(case.wd), "--seed", str(L.SEED)] + (["--hostData"] if host else []))
    run = finetune_lut.FinetuneRun(opt, log=lines.append)
    seen = []      # the output of every forward the run's module makes
    run.net.register_forward_hook(lambda mod, args, out: seen.append(out.detach().clone()))
    return run, lines, seen, train, exp


def host(t):
    return t.detach().cpu().numpy().copy()


def adam_state(run, params):
    out = {}
    for k, p in params.items():
        st = run.optim.state.get(p)
        out[k] = (host(st["exp_avg"]), host(st["exp_avg_sq"]), int(st["step"].item())) if st else (np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32), 0)
    return out


@pytest.mark.parametrize("name", list(L.CASES))
def test_every_step_from_the_state_the_device_holds(tmp_path, name):
    case = L.CASES[name]
    run, lines, seen, train, exp = make_run(case, tmp_path)
    second = finetune_lut.CropProvider(train, case.scale, case.crop, case.batch, seed=L.SEED)
    restated = L.batches(case)
    params = {k: getattr(run.net, "weight_" + k) for k in L.keys(case)}
    assert len(list(run.net.parameters())) == len(params)
    reads, worst = [], {"loss": 0.0, "p": (0.0, 0.0), "exp_avg": (0.0, 0.0), "exp_avg_sq": (0.0, 0.0)}
    for i in range(1, case.K + 1):
        # 1. before the step
        w, state, lr = {k: host(p) for k, p in params.items()}, adam_state(run, params), run.optim.param_groups[0]["lr"]
        im_t, lb_t = second.next()
        im, lb = host(im_t), host(lb_t)
        assert np.array_equal(im, restated[i - 1][0]) and np.array_equal(lb, restated[i - 1][1])      # the batches test_ft_loop_cpu.py ran
        with torch.no_grad():
            again = host(run.net(im_t))
        del seen[:]
        # 2. the step
        run.step()
        loss = float(run.loss_buf[i - 1].item())
        reads.append(loss)
        assert all(p.grad is not None for p in params.values())
        grads = {k: host(p.grad) for k, p in params.items()}
        w1, state1 = {k: host(p) for k, p in params.items()}, adam_state(run, params)
        # 3. forward: no tolerance
        r = L.oracle_step(case, w, im, lb, torch.float64)
        assert len(seen) == 1
        for got, what in ((host(seen[0]), "the step's forward"), (again, "net(im) under no_grad")):
            # compared as bytes: the module's closing x / 255.0 is torch's, which multiplies by a rounded 1 / 255 on the device, so
            # the float is k / 255 to within one float32 ulp and times 255 it is k to within 255 * 2^-24 k / 255 < 2e-5
            g255 = got.astype(np.float64) * 255.0
            bad = int((np.rint(g255) != r.out).sum())
            assert bad == 0, "%s step %d, %s: %d of %d pixels differ from the oracle" % (name, i, what, bad, r.out.size)
            assert np.abs(g255 - r.out).max() < 2e-5
        assert np.array_equal(host(seen[0]), again)
        # 4. loss
        rel = abs(loss - r.loss) / r.loss
        worst["loss"] = max(worst["loss"], rel)
        print("%s step %d loss %.9g oracle %.9g rel %.3g" % (name, i, loss, r.loss, rel))
        assert rel <= 4 * L.LOSS_F32_REL, (name, i, loss, r.loss, rel)
        # 5. gradients
        for k in params:
            close(grads[k], r.grads[k], "%s step %d grad %s" % (name, i, k))
            assert not grads[k][r.beyond[k]].any(), (name, i, k, "gradient beyond the quantiser's clamp")
        # 6. optimiser and schedule
        want_lr = L.lr_at(case, i)
        assert lr == pytest.approx(want_lr, rel=1e-15, abs=0.0), (name, i, lr, want_lr)
        for k in params:
            m, v, step = state[k]
            ref = L.adam_step(w[k], grads[k], m, v, step, want_lr, case.wd)
            cpu = L.torch_adam_step(w[k], grads[k], m, v, step, want_lr, case.wd, torch.float32)
            assert state1[k][2] == ref[3] == cpu[3] == i, (name, i, k, state1[k][2])
            for kind, got, c32, r64 in (("p", w1[k], cpu[0], ref[0]), ("exp_avg", state1[k][0], cpu[1], ref[1]), ("exp_avg_sq", state1[k][1], cpu[2], ref[2])):
                cpu_ulps, dev_ulps = float(L.ulps32(c32, r64).max()), float(L.ulps32(got, r64).max())
                bar = max(1.0, 2 * cpu_ulps)
                worst[kind] = (max(worst[kind][0], dev_ulps), max(worst[kind][1], cpu_ulps))
                assert dev_ulps <= bar, "%s step %d %s of %s: the device is %.3g float32 ulps from float64 Adam, the CPU's float32 Adam %.3g" % (
                    name, i, kind, k, dev_ulps, cpu_ulps)
                # the driver's optimiser (mulut_amd.finetune.Adam) does its arithmetic in float64 and rounds once: half an ulp, whatever the
                # bar above allows (the CPU's float32 Adam is hundreds of ulps off on an element that lands near zero)
                assert dev_ulps <= 0.5 + 1e-3, (name, i, kind, k, dev_ulps)
    print("%s largest: loss rel %.3g; (device ulps, CPU float32 ulps) from float64 Adam: p %s exp_avg %s exp_avg_sq %s" % (
        name, worst["loss"], worst["p"], worst["exp_avg"], worst["exp_avg_sq"]))
    # 7. after K steps
    losses = run.finish()
    assert losses == reads
    shown = [ln for ln in lines if "Iter:" in ln]
    points = [i for i in range(1, case.K + 1) if i % L.DISPLAY_STEP == 0]
    assert len(shown) == len(points)
    for ln, i in zip(shown, points):
        head = "{} | Iter:{:6d}, Sample:{:6d}, GPixel:{:.2e}, rT:".format(exp, i, i * case.batch, sum(reads[i - L.DISPLAY_STEP:i]) / L.DISPLAY_STEP)
        assert ln.startswith(head), (ln, head)
    assert lines[-1] == "Finetuned LUT saved to {}".format(exp)
    for k in params:
        saved = np.load(os.path.join(exp, "LUT_ft_x{}_{}bit_int8_{}.npy".format(case.scale, case.interval, k)))
        assert saved.dtype == np.int8 and np.array_equal(saved, np.round(np.clip(w1[k], -1, 1) * 127).astype(np.int8)), k      # sr/3_finetune_lut.py:168
        assert np.array_equal(w1[k], host(params[k]))                      # finish() takes no further step


def test_adam_kernel_over_more_tensors_than_one_launch_takes():
    """mulut_amd.finetune.Adam on 35 tensors (mulut_ft_adam launches 32 at a time) of 1 .. 1.3 M elements (the grid-stride loop starts
    beyond 2^20), with weight decay, three steps from random moments-free state: every stored value is float64 Adam's rounded once.
    Tensors without a gradient are left alone and keep no state."""
    from mulut_amd.finetune import Adam
    rng = np.random.default_rng(35)
    sizes = [1, 2, 255, 256, 257, 1000, 4097, 83521 * 16] + [int(v) for v in rng.integers(1, 3000, 27)]
    ps = [torch.nn.Parameter(torch.from_numpy(rng.uniform(-1, 1, n).astype(np.float32)).cuda()) for n in sizes]
    idle = torch.nn.Parameter(torch.ones(7, device="cuda"))
    opt = Adam(ps + [idle], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    ref = [(host(p).astype(np.float64), np.zeros(n), np.zeros(n), 0) for p, n in zip(ps, sizes)]
    for step in range(1, 4):
        lr = 1e-2 / step
        opt.param_groups[0]["lr"] = lr
        gs = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-9, -2, n)).astype(np.float32) for n in sizes]
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g).cuda()
        before = [(host(p), host(opt.state[p]["exp_avg"]), host(opt.state[p]["exp_avg_sq"])) if step > 1 else (host(p), np.zeros(n, np.float32), np.zeros(n, np.float32))
                  for p, n in zip(ps, sizes)]
        opt.step()
        for t, (p, g, b) in enumerate(zip(ps, gs, before)):
            want = L.adam_step(b[0], g, b[1], b[2], step - 1, lr, 1e-2)
            st = opt.state[p]
            assert int(st["step"].item()) == step
            for got, w64, what in ((host(p), want[0], "p"), (host(st["exp_avg"]), want[1], "exp_avg"), (host(st["exp_avg_sq"]), want[2], "exp_avg_sq")):
                assert float(L.ulps32(got, w64).max()) <= 0.5 + 1e-3, (t, sizes[t], step, what)
    assert torch.equal(idle.detach(), torch.ones(7, device="cuda")) and len(opt.state[idle]) == 0


def test_the_two_providers_start_the_same_run(tmp_path):
    """case A with the batches cut on the device and on the host: the first step's forward bytes and loss are bit-equal (the same
    batch, a deterministic forward).  Later steps are not compared: the atomics reorder the gradients' sums."""
    case = L.CASES["A"]
    first = []
    for host_data in (False, True):
        sub = tmp_path / ("host" if host_data else "device")
        sub.mkdir()
        run, lines, seen, train, exp = make_run(case, sub, host=host_data)
        assert isinstance(run.data, finetune_lut.CropProvider if host_data else finetune_lut.DeviceCropProvider)
        run.step()
        assert len(seen) == 1
        first.append((host(seen[0]), host(run.loss_buf[:1])))
    assert first[0][0].any() and np.array_equal(first[0][0], first[1][0])
    assert first[0][1].tobytes() == first[1][1].tobytes()


# ------------------------------------------------------------------------------------------------------------------ validation
def write_val_dir(root):
    """{root}/Set5/{HR, LR_bicubic/X4}: the three smallest Set5 pairs (symlinks), a grey pair, and an RGB pair whose HR is no
    multiple of the scale in either dimension (LR: the modcropped size / 4).  Stems with a '_': the reference names a result after
    the last '_'-token."""
    from mulut_amd.synth import natural_frames
    hr_dir, lr_dir = os.path.join(str(root), "Set5", "HR"), os.path.join(str(root), "Set5", "LR_bicubic", "X4")
    os.makedirs(hr_dir)
    os.makedirs(lr_dir)
    src = os.path.join(GOLDEN, "Set5")
    sizes = sorted((Image.open(os.path.join(src, "LR_bicubic", "X4", fn)).size, fn) for fn in os.listdir(os.path.join(src, "HR")))
    small = [fn for (w, h), fn in sizes if max(w, h) <= 72]
    assert len(small) == 3
    for fn in small:
        os.symlink(os.path.join(src, "HR", fn), os.path.join(hr_dir, fn))
        os.symlink(os.path.join(src, "LR_bicubic", "X4", fn), os.path.join(lr_dir, fn))
    grey = natural_frames(1, 48, 44, 1, seed=61)[0, :, :, 0]
    Image.fromarray(grey).save(os.path.join(hr_dir, "zz_grey.png"))
    Image.fromarray(grey.reshape(12, 4, 11, 4).mean(axis=(1, 3)).round().astype(np.uint8)).save(os.path.join(lr_dir, "zz_grey.png"))
    odd = natural_frames(1, 62, 55, 3, seed=62)[0]                          # modcrop: 60 x 52
    Image.fromarray(odd).save(os.path.join(hr_dir, "zz_odd.png"))
    Image.fromarray(odd[:60, :52].reshape(15, 4, 13, 4, 3).mean(axis=(1, 3)).round().astype(np.uint8)).save(os.path.join(lr_dir, "zz_odd.png"))
    return str(root), sorted(os.listdir(hr_dir))


def test_bytes_survive_the_devices_division_and_product():
    """valid_steps rounds net(x) * 255 (sr/3_finetune_lut.py:54).  The module's x / 255.0 is a product with a rounded 1 / 255 on the
    device, and times 255 about half of the bytes come back one float32 ulp off: the round() is what gives the byte back.  (All of
    those ulps are upward -- in float32, (k * fl(1 / 255)) * 255 >= k for every byte k -- so a floor() in its place writes the same
    files on this device; a ceil() would not.  Recorded, not asserted: the driver relies on round() alone.)"""
    k = torch.arange(256, dtype=torch.float32, device="cuda")
    v = (k / 255.0) * 255.0
    print("bytes whose round trip is inexact: %d of 256, %d of them below" % (int((v != k).sum()), int((v < k).sum())))
    assert torch.equal(torch.round(v), k) and float((v - k).abs().max()) < 2e-5


@pytest.mark.parametrize("interval", [4, 5])
def test_validation_loop_writes_the_oracles_bytes_and_scores_them(tmp_path, interval):
    """valid_steps on MuLUT with the shipped LUT_ft tables, and on MuLUTInterval at interval 5 with make_table tables: every PNG is
    round(clip(oracle forward * 255)) of its LR under the reference's file name; opt.valResults is mulut_amd/metrics.py on those
    bytes against the modcropped HR (grey replicated) within the bars of test_gpu_eval.py; the log line is the reference's format
    of their means."""
    from mulut_amd.finetune import MuLUT, MuLUTInterval
    from mulut_amd.metrics import modcrop, psnr, rgb2ycbcr, ssim
    from oracle import ft_torch
    val, files = write_val_dir(tmp_path / "bench")
    exp = tmp_path / "exp"
    exp.mkdir()
    tabs = {}
    for s in (1, 2):
        for m in "sdy":
            if interval == 4:
                t = np.load(os.path.join(GOLDEN, "luts", "LUT_ft_x4_4bit_int8_s%d_%s.npy" % (s, m)))
            else:
                t = A.make_table(np.random.default_rng(10 * s + ord(m)), interval, 16 if s == 2 else 1, True)
            np.save(exp / ("LUT_x4_%dbit_int8_s%d_%s.npy" % (interval, s, m)), t)
            tabs["s%d_%s" % (s, m)] = torch.from_numpy(t.reshape(-1, 16 if s == 2 else 1).astype(np.float32) / 127.0)
    net = (MuLUT if interval == 4 else MuLUTInterval)(str(exp), 2, list("sdy"), upscale=4, interval=interval).cuda()
    opt = argparse.Namespace(valDir=val, valoutDir=str(tmp_path / "out"), scale=4, debug=True)
    lines = []
    net.train()
    ret = finetune_lut.valid_steps(net, opt, 7, lines.append)
    assert net.training
    assert list(opt.valResults) == ["Set5"] and opt.valResults["Set5"].shape == (5, 2) and opt.valResults["Set5"].dtype == np.float64
    assert sorted(os.listdir(os.path.join(opt.valoutDir, "Set5"))) == sorted(fn[:-4].split("_")[-1] + "_lutft.png" for fn in files)
    for n, fn in enumerate(files):
        lr = np.array(Image.open(os.path.join(val, "Set5", "LR_bicubic", "X4", fn)))
        hr = modcrop(np.array(Image.open(os.path.join(val, "Set5", "HR", fn))), 4)
        if lr.ndim == 2:                                                   # sr/data.py:145-158: each on its own
            lr = np.stack([lr] * 3, 2)
        if hr.ndim == 2:
            hr = np.stack([hr] * 3, 2)
        assert (lr.shape[0] * 4, lr.shape[1] * 4) == hr.shape[:2]          # :163-165
        with torch.no_grad():
            x = torch.from_numpy(np.ascontiguousarray(lr.transpose(2, 0, 1)[None]).astype(np.float32) / 255.0)
            out = ft_torch.forward(tabs, x, 2, "sdy", 4, interval).numpy()[0].transpose(1, 2, 0) * 255.0
        want = np.round(np.clip(out, 0, 255)).astype(np.uint8)             # sr/3_finetune_lut.py:54
        got = np.array(Image.open(os.path.join(opt.valoutDir, "Set5", fn[:-4].split("_")[-1] + "_lutft.png")))
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), "%s: %d of %d bytes differ" % (fn, int((got != want).sum()), want.size)
        left, right = rgb2ycbcr(want)[:, :, 0], rgb2ycbcr(hr)[:, :, 0]
        p, s = opt.valResults["Set5"][n]
        assert p == pytest.approx(float(psnr(left, right, 4)), abs=1e-4), fn
        assert s == pytest.approx(ssim(left, right), abs=1e-10), fn
    means = opt.valResults["Set5"].mean(0)
    assert list(ret) == ["Set5"] and ret["Set5"] == pytest.approx((float(means[0]), float(means[1])), rel=1e-14, abs=0.0)
    assert lines == ['Iter {} | Dataset {} | AVG PSNR: {:02f}, AVG: SSIM: {:04f}'.format(7, "Set5", means[0], means[1])]
