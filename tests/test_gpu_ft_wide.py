"""Fine-tuning mode lists with the 4 x 4 patterns e, h, o on the GPU (mulut_ft_wide_stage_forward / _backward: the backward kernels
of mulut_ft.hip and mulut_ft_interval.hip instantiated with a 3-pixel halo of the input gradient; mulut_amd.finetune.MuLUTWide;
the driver).

The reference of every test is oracle/ft_torch.py with the taps of e, h, o added at run time (tests/ft_wide_cases.wide_oracle,
held to the NumPy restatement of a pass by tests/test_ft_wide_cpu.py) -- never the code under test:
  1. every exact case of tests/ft_wide_cases.py bit for bit: out, the clamp mask, grad_x and every grad_wq (no tolerance);
  2. a list of s, d, y through the new entry points gives the bytes of the existing entry points;
  3. the module on float data with weights off the grid, at the float bars of test_gpu_ft_interval.py::test_more_shapes_vs_cpu_oracle;
  4. the bs 256 x 48 x 48 batch of natural crops, bars set from the reference side;
  5. the driver end to end."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

torch = pytest.importorskip("torch")

import ft_exact_cases as fx      # noqa: E402
import ft_wide_cases as fw       # noqa: E402

pytestmark = pytest.mark.gpu

# bs-256 bars of test 4, set from the REFERENCE side as BS256_BARS of test_gpu_ft_interval.py was.  The extended oracle's float32
# table gradients of this test's own batch (2-stage eho x4, the seeded tables below, 256 natural crops) were computed on the CPU
# with the crops in the given order, in reversed order and in one seeded shuffle (tools/ft_err_probe.py --modes eho --interval N
# --orderings): the same sums in another order.  Worst difference between two of the three orderings, over all six tables:
#   interval 4: norm-wise 7.610e-6 of the largest element, element-wise 9.197e-6 on the elements above 1 % of it
#   interval 5: norm-wise 1.049e-5,                        element-wise 1.387e-5
#   interval 6: norm-wise 1.731e-5,                        element-wise 2.057e-5
# (grad_x: 0 -- a crop's input gradient does not depend on the order of the crops -- so grad_x keeps the general bars.)  The bar is
# twice that: three orderings are a small sample of what an ordering can do, and the GPU's sums are one more ordering.
# Measured on the GPU (MI355X, worst table of one run of this test, which prints every figure; the order of the atomics changes them
# from run to run): interval 4 norm-wise 4.57e-6, element-wise 7.01e-6; interval 5 8.46e-6 and 8.47e-6; interval 6 1.85e-5 and
# 1.90e-5.  grad_x at bs 256: norm-wise 3.1e-7, element-wise 1.04e-5 (general bars).
BS256_BARS = {4: (2 * 7.610e-6, 2 * 9.197e-6), 5: (2 * 1.049e-5, 2 * 1.387e-5), 6: (2 * 1.731e-5, 2 * 2.057e-5)}      # interval -> (norm-wise, element-wise)
GENERAL_BARS = (2e-5, 5e-5)      # norm-wise over ALL elements, element-wise above 1 % of the maximum (test_more_shapes_vs_cpu_oracle)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _wide_forward(lib, case, wq, x):
    B, C, H, W = case.shape
    u = case.u
    out = torch.full((B, C, H * u, W * u), float("nan"), dtype=torch.float32, device="cuda")
    mask = torch.full(case.shape, -1, dtype=torch.int16, device="cuda")
    rc = lib.mulut_ft_wide_stage_forward(0, case.interval, _ptrs(wq), case.modes.encode(), case.last, u, x.data_ptr(), B, C, H, W,
                                         out.data_ptr(), mask.data_ptr(), _stream())
    assert rc == 0, rc
    return out, mask


def _wide_backward(lib, case, wq, x, gout, mask):
    B, C, H, W = case.shape
    gw = [torch.zeros_like(w) for w in wq]
    gx = torch.zeros_like(x)
    rc = lib.mulut_ft_wide_stage_backward(0, case.interval, _ptrs(wq), case.modes.encode(), case.last, case.u, x.data_ptr(), gout.data_ptr(),
                                          mask.data_ptr(), B, C, H, W, _ptrs(gw), gx.data_ptr(), _stream())
    assert rc == 0, rc
    return gx.cpu().numpy(), [g.cpu().numpy() for g in gw]


# ---------------------------------------------------------------------------------------------------------------- 1. exact bytes
@pytest.mark.parametrize("case", fw.CASES, ids=lambda c: c.name)
def test_wide_stage_kernels_equal_the_integer_reference(case):
    from mulut_amd import _native
    lib = _native.load()
    case.build()
    try:
        ref = fw.reference(case)      # asserts the exactness cap and the case's reach, on the extended oracle alone
        wq = [torch.from_numpy(t.astype(np.float32)).cuda() for t in case.tables]
        x, gout = torch.from_numpy(case.x).cuda(), torch.from_numpy(case.gout).cuda()
    finally:
        case.tables = case.x = case.gout = None
    print(case.name, "sum |terms| * q =", ref.cap, ref.reach)
    if case.shape == (1, 1, 1, 1):
        assert ref.cap > 0      # the one site is not clamped away
    bad = []
    out, mask = _wide_forward(lib, case, wq, x)
    bad.append(fx.describe(case, "out", out.cpu().numpy(), ref.out, q=1))
    bits = mask.cpu().numpy().view(np.uint16) & np.uint16((1 << case.u * case.u) - 1)
    bad.append(fx.describe(case, "inside, bits 0..u*u-1 (1/q = one mask value)", bits.astype(np.float32), ref.inside.astype(np.int64), q=1))
    runs = [_wide_backward(lib, case, wq, x, gout, mask) for _ in range(2)]      # twice in a row into zeroed buffers
    gx, gw = runs[0]
    bad.append(fx.describe(case, "grad_x", gx, ref.gx_num))
    for m in range(case.M):
        bad.append(fx.describe(case, "grad_wq[%d]" % m, gw[m], ref.gw_num[m]))
    for a, b, what in zip([runs[0][0]] + runs[0][1], [runs[1][0]] + runs[1][1], ["grad_x"] + ["grad_wq[%d]" % m for m in range(case.M)]):
        if not np.array_equal(a, b):
            bad.append("%s: %s differs between two runs of one backward in %d elements" % (case.name, what, int((a != b).sum())))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------- 2. the new entry points on a narrow list
@pytest.mark.parametrize("interval", fw.INTERVALS)
@pytest.mark.parametrize("u,last", [(1, 0), (4, 1)])
def test_narrow_list_through_the_wide_entry_points_gives_the_old_bytes(interval, u, last):
    """sdy goes to the halo-2 launch of its interval: out, mask, grad_x and grad_wq are those of mulut_ft_stage_*_mask (interval 4) /
    mulut_ft_interval_stage_* (5, 6), and both are the reference's (an exact case: the order of the atomics cannot show)."""
    from mulut_amd import _native
    lib = _native.load()
    case = fx.Case(interval, u, last, "sdy", (2, 1, 13, 10), "noise").build()
    ref = fx.reference(case)
    wq = [torch.from_numpy(t.astype(np.float32)).cuda() for t in case.tables]
    x, gout = torch.from_numpy(case.x).cuda(), torch.from_numpy(case.gout).cuda()
    B, C, H, W = case.shape
    out, mask = _wide_forward(lib, case, wq, x)
    gx, gw = _wide_backward(lib, case, wq, x, gout, mask)
    out0 = torch.full_like(out, float("nan"))
    mask0 = torch.full_like(mask, -1)
    gw0 = [torch.zeros_like(w) for w in wq]
    gx0 = torch.zeros_like(x)
    if interval == 4:
        assert lib.mulut_ft_stage_forward_mask(0, _ptrs(wq), b"sdy", last, u, x.data_ptr(), B, C, H, W, out0.data_ptr(), mask0.data_ptr(), _stream()) == 0
        assert lib.mulut_ft_stage_backward_mask(0, _ptrs(wq), b"sdy", last, u, x.data_ptr(), gout.data_ptr(), mask0.data_ptr(), B, C, H, W,
                                                _ptrs(gw0), gx0.data_ptr(), _stream()) == 0
    else:
        assert lib.mulut_ft_interval_stage_forward(0, interval, _ptrs(wq), b"sdy", last, u, x.data_ptr(), B, C, H, W, out0.data_ptr(),
                                                   mask0.data_ptr(), _stream()) == 0
        assert lib.mulut_ft_interval_stage_backward(0, interval, _ptrs(wq), b"sdy", last, u, x.data_ptr(), gout.data_ptr(), mask0.data_ptr(),
                                                    B, C, H, W, _ptrs(gw0), gx0.data_ptr(), _stream()) == 0
    assert torch.equal(out, out0) and torch.equal(mask, mask0)
    assert np.array_equal(gx, gx0.cpu().numpy())
    for m in range(3):
        assert np.array_equal(gw[m], gw0[m].cpu().numpy()), m
    assert fx.describe(case, "out", out.cpu().numpy(), ref.out, q=1) is None and fx.describe(case, "grad_x", gx, ref.gx_num) is None
    for m in range(3):
        assert fx.describe(case, "grad_wq[%d]" % m, gw[m], ref.gw_num[m]) is None


# --------------------------------------------------------------------------------------------------- 3. the module on float data
def synthetic_lut(interval, stage, mode, vnum):      # as tests/test_gpu_ft_interval.py
    rng = np.random.default_rng(1000 * interval + 17 * stage + ord(mode))
    return rng.integers(-128, 128, size=((2 ** (8 - interval) + 1) ** 4, vnum), dtype=np.int8)


def save_tables(folder, stages, modes, scale, interval):
    for s in range(stages):
        for m in set(modes):
            np.save(os.path.join(str(folder), "LUT_x%d_%dbit_int8_s%d_%s.npy" % (scale, interval, s + 1, m)),
                    synthetic_lut(interval, s + 1, m, scale * scale if s + 1 == stages else 1))


def natural_batch(rng, shape):      # as tests/test_gpu_ft_interval.py
    from mulut_amd.synth import natural_frames
    big = natural_frames(1, 1080, 1920, 1, 11)[0, :, :, 0]
    ys, xs = rng.integers(0, 1080 - shape[2], shape[0]), rng.integers(0, 1920 - shape[3], shape[0])
    return np.stack([big[a:a + shape[2], b:b + shape[3]] for a, b in zip(ys, xs)])[:, None].astype(np.float32) / np.float32(255)


def errors(g, r):
    """(norm-wise, element-wise) error of g against r, as tests/test_gpu_ft_interval.py"""
    scale = max(float(np.abs(r).max()), 1e-30)
    sig = np.abs(r) > 0.01 * scale
    return float(np.abs(g - r).max()) / scale, float((np.abs(g - r)[sig] / np.abs(r)[sig]).max()) if sig.any() else 0.0


def module_and_oracle(tmp_path, interval, stages, modes, scale, x, tgt, off_grid, rng):
    """MuLUTWide on the GPU and ft_torch.forward (extended) on the CPU on the same floats: (forward difference, [(name, gpu grad, oracle grad)])"""
    from mulut_amd.finetune import MuLUTWide
    save_tables(tmp_path, stages, modes, scale, interval)
    net = MuLUTWide(str(tmp_path), stages, modes, upscale=scale, interval=interval).cuda()
    keys = ["s%d_%s" % (s + 1, m) for s in range(stages) for m in modes]
    wcpu = {}
    with torch.no_grad():
        for key in keys:
            p = getattr(net, "weight_" + key)
            w = p.cpu().numpy()
            if off_grid:      # as after an optimiser step: no weight is k / 127, some leave [-1, 1] (test_gpu_ft_exact.py)
                w = (w + rng.uniform(-0.45, 0.45, w.shape).astype(np.float32) / np.float32(127)).astype(np.float32)
                w = np.where(rng.random(w.shape) < 0.05, w * np.float32(1.4), w).astype(np.float32)
                p.copy_(torch.from_numpy(w))
            wcpu[key] = torch.from_numpy(w.copy()).requires_grad_(True)
    xc = torch.from_numpy(x).requires_grad_(True)
    with fw.wide_oracle():
        yc = fw.ft_torch.forward(wcpu, xc, stages, modes, scale, interval)
        torch.nn.functional.mse_loss(yc, torch.from_numpy(tgt)).backward()
    xg = torch.from_numpy(x).cuda().requires_grad_(True)
    yg = net(xg)
    torch.nn.functional.mse_loss(yg, torch.from_numpy(tgt).cuda()).backward()
    fwd = float(np.abs(yg.detach().cpu().numpy() - yc.detach().numpy()).max())
    pairs = [("gx", xg.grad.cpu().numpy(), xc.grad.numpy())]
    pairs += [(k, getattr(net, "weight_" + k).grad.cpu().numpy(), w.grad.numpy()) for k, w in wcpu.items()]
    return fwd, pairs


MODULE_CASES = [
    # stages, modes, scale, shape
    (2, "eho", 4, (2, 1, 9, 7)),
    (3, "sdyeho", 2, (1, 3, 5, 6)),
    (1, "h", 3, (2, 1, 9, 7)),
]


@pytest.mark.parametrize("interval", fw.INTERVALS)
@pytest.mark.parametrize("stages,modes,scale,shape", MODULE_CASES)
def test_module_with_off_grid_weights_vs_cpu_oracle(tmp_path, interval, stages, modes, scale, shape):
    rng = np.random.default_rng(stages * 100 + scale * 10 + len(modes) + interval)
    x = rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)
    tgt = rng.random((shape[0], shape[1], shape[2] * scale, shape[3] * scale), dtype=np.float32)
    fwd, pairs = module_and_oracle(tmp_path, interval, stages, modes, scale, x, tgt, True, rng)
    print(interval, modes, scale, shape, "forward %.3g" % fwd)
    for what, g, r in pairs:
        print(interval, modes, scale, shape, what, "norm-wise %.3g element-wise %.3g" % errors(g, r))
    assert fwd <= 1e-5
    for what, g, r in pairs:
        en, ee = errors(g, r)
        assert en <= GENERAL_BARS[0], (what, en)
        assert ee <= GENERAL_BARS[1], (what, ee)
    assert float(np.abs(pairs[1][2]).max()) > 0 and float(np.abs(pairs[0][2]).max()) > 0      # the case has gradients at all


# ------------------------------------------------------------------------------------------------------- 4. bs 256 natural crops
@pytest.mark.parametrize("interval", fw.INTERVALS)
def test_bs256_natural_crops_vs_cpu_oracle(tmp_path, interval):
    stages, modes, scale, shape = 2, "eho", 4, (256, 1, 48, 48)
    rng = np.random.default_rng(stages * 100 + scale * 10 + len(modes) + interval)      # tools/ft_err_probe.py draws the same batch
    x = natural_batch(np.random.default_rng(1), shape)
    tgt = rng.random((shape[0], shape[1], shape[2] * scale, shape[3] * scale), dtype=np.float32)
    fwd, pairs = module_and_oracle(tmp_path, interval, stages, modes, scale, x, tgt, False, rng)
    print(interval, "forward %.3g" % fwd)
    for what, g, r in pairs:
        print(interval, modes, shape, what, "norm-wise %.3g element-wise %.3g" % errors(g, r))
    assert fwd <= 1e-5
    for what, g, r in pairs:
        en, ee = errors(g, r)
        bars = GENERAL_BARS if what == "gx" else BS256_BARS[interval]
        assert en <= bars[0], (what, en, bars)
        assert ee <= bars[1], (what, ee, bars)
    assert float(np.abs(pairs[1][2]).max()) > 0


# -------------------------------------------------------------------------------------------------------------------- 5. driver
def _seeded_tables(exp, modes, interval):
    """Tables with something to learn and every stage's input on the whole byte range: the smooth ramp tables of tests/reach_cases.py
    (the kind the inference tests of the wide patterns use) with seeded noise."""
    import reach_cases as rc
    for s in (1, 2):
        for i, m in enumerate(modes):
            t = rc.table("ramp", interval, 16 if s == 2 else 1, seed=10 * s + i, final=s == 2)
            np.save(exp / ("LUT_x4_%dbit_int8_s%d_%s.npy" % (interval, s, m)), np.clip(t, -127, 127).astype(np.int8))


def test_finetune_driver_with_wide_modes_reduces_loss_and_writes_luts(tmp_path):
    """sr/3_finetune_lut.py --modes eho on the Set5 pairs: the loss goes down, the LUT_ft files appear in the reference's int8 format and
    load back into the inference engine, which upscales a Set5 image with them."""
    from PIL import Image
    from mulut_amd import finetune_lut, MuLUTEngine, load_lut_dict
    exp = tmp_path / "exp"
    exp.mkdir()
    _seeded_tables(exp, "eho", 4)
    losses = finetune_lut.main(["--stages", "2", "--modes", "eho", "--interval", "4", "-e", str(exp), "--trainDir", os.path.join(GOLDEN, "Set5"),
                                "--batchSize", "16", "--cropSize", "24", "--totalIter", "60", "--displayStep", "20",
                                "--lr0", "1e-3", "--seed", "0", "--valDir", str(tmp_path / "none"), "--valStep", "1000"])
    print("loss, first and last 15 iterations: %.5g %.5g" % (np.mean(losses[:15]), np.mean(losses[-15:])))
    assert len(losses) == 60 and np.mean(losses[-15:]) < np.mean(losses[:15])
    for s in (1, 2):
        for m in "eho":
            t = np.load(exp / ("LUT_ft_x4_4bit_int8_s%d_%s.npy" % (s, m)))
            assert t.dtype == np.int8 and t.shape == (17 ** 4, 16 if s == 2 else 1)
    luts = load_lut_dict(str(exp), 2, "eho", 4, 4, "LUT_ft")
    eng = MuLUTEngine(0).configure(2, "eho", 4, 4).set_lut_dict(luts)
    lr_dir = os.path.join(GOLDEN, "Set5", "LR_bicubic", "X4")
    img = np.array(Image.open(os.path.join(lr_dir, sorted(os.listdir(lr_dir))[0])))
    out = eng.pipeline(torch.from_numpy(np.ascontiguousarray(img)).cuda())
    assert out.shape == (img.shape[0] * 4, img.shape[1] * 4, 3) and out.dtype == torch.uint8
    eng.close()


def test_finetune_driver_one_step_at_interval_6_with_all_six_patterns(tmp_path):
    from mulut_amd import finetune_lut, load_lut_dict
    exp = tmp_path / "exp"
    exp.mkdir()
    _seeded_tables(exp, "sdyeho", 6)
    losses = finetune_lut.main(["--stages", "2", "--modes", "sdyeho", "--interval", "6", "-e", str(exp), "--trainDir", os.path.join(GOLDEN, "Set5"),
                                "--batchSize", "8", "--cropSize", "24", "--totalIter", "1", "--displayStep", "1",
                                "--lr0", "1e-3", "--seed", "0", "--valDir", str(tmp_path / "none"), "--valStep", "1000"])
    assert len(losses) == 1 and np.isfinite(losses[0])
    luts = load_lut_dict(str(exp), 2, "sdyeho", 4, 6, "LUT_ft")
    assert luts["s2_e"].dtype == np.int8 and luts["s2_e"].shape == (625, 16) and luts["s1_o"].shape == (625, 1)
