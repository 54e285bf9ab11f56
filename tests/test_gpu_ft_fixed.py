"""The bit-reproducible (fixed-point) backward of a fine-tune stage on the GPU: mulut_ft_exact_stage_backward (mulut_ft_exact.hip),
``MuLUT(..., deterministic=True)`` and the driver's ``--deterministic``.

The reference of the exact tests is the host model (tests/host_emul/ft_exact_host.cpp through tests/ft_fixed_cases.py, held to the
oracle's autograd by tests/test_ft_fixed_cpu.py) -- never the code under test -- and equality means EXACT: torch.equal on the raw
bits of every grad_wq[m] and of grad_x.
  1. every case of ft_fixed_cases.py: the model's bytes, the same bytes from a second call, and from a batch in another order;
  2. an all-zero grad_out writes nothing; destinations with prior contents come out as prior + value, rounded once;
  3. a non-blocking side stream; a captured graph replayed after grad_out was rewritten in place;
  4. the yardstick: the fast (float-atomic) backward against the exact one on natural crops, at the bar of ft_grad_bar.py;
  5. the module twice, the driver twice: identical parameters, tables and losses."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

torch = pytest.importorskip("torch")

import ft_fixed_cases as fc      # noqa: E402
import ft_grad_bar               # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from mulut_amd import _native
    return _native.load()


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def bits(t):
    return t.contiguous().view(torch.int32)


class Call:
    """The device buffers of one call of a case; run() queues it on the current stream"""

    def __init__(self, case, perm=None, prior=None):
        case.build()
        self.case = case
        sel = list(perm) if perm is not None else slice(None)
        self.wq = [torch.from_numpy(t).cuda() for t in case.tables]
        self.x = torch.from_numpy(np.ascontiguousarray(case.x[sel])).cuda()
        self.gout = torch.from_numpy(np.ascontiguousarray(case.gout[sel])).cuda()
        self.inside = torch.from_numpy(np.ascontiguousarray(case.inside[sel]).view(np.int16)).cuda()
        if prior is None:
            self.gw = [torch.zeros_like(w) for w in self.wq]
            self.gx = torch.zeros_like(self.x)
        else:
            self.gw = [torch.from_numpy(np.ascontiguousarray(g)).cuda() for g in prior[0]]
            self.gx = torch.from_numpy(np.ascontiguousarray(prior[1])).cuda()
        B, C, H, W = case.shape
        self.need = _lib().mulut_ft_exact_ws_bytes(case.interval, case.modes.encode(), case.u, B, C, H, W)
        assert self.need == 8 * (1 + case.M * fc.rows_of(case.interval) * case.u ** 2 + B * C * H * W)
        # the workspace's content on entry is irrelevant: it starts as noise, and a second call finds the first one's sums
        self.ws = torch.randint(-2 ** 62, 2 ** 62, (self.need // 8,), dtype=torch.int64, device="cuda")

    def run(self):
        c = self.case
        B, C, H, W = c.shape
        rc = _lib().mulut_ft_exact_stage_backward(0, c.interval, _ptrs(self.wq), c.modes.encode(), c.last, c.u, self.x.data_ptr(), self.gout.data_ptr(),
                                                  self.inside.data_ptr(), B, C, H, W, _ptrs(self.gw), self.gx.data_ptr(), self.ws.data_ptr(), self.need,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        return self

    def zero(self):
        for g in self.gw:
            g.zero_()
        self.gx.zero_()

    def results(self):
        return [bits(g).clone() for g in self.gw] + [bits(self.gx).clone()]


def differences(case, got, want):
    """one line per buffer whose bits differ from the model's"""
    out = []
    for m in range(case.M + 1):
        w = torch.from_numpy((want.gw[m] if m < case.M else want.gx).view(np.int32).reshape(-1))
        g = got[m].cpu().reshape(-1)
        if not torch.equal(g, w):
            bad = (g != w).nonzero().reshape(-1)
            i = int(bad[0])
            out.append("%s %s: %d of %d elements differ, first at %d: got %r, model %r" % (
                case.name, "grad_wq[%d]" % m if m < case.M else "grad_x", len(bad), len(w), i,
                float(g[i:i + 1].view(torch.float32)), float(w[i:i + 1].view(torch.float32))))
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. exact bytes
@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_kernels_give_the_host_models_bytes_in_any_order(case):
    try:
        want = fc.expected(case)
        call = Call(case).run()
        first = call.results()
        call.zero()
        second = call.run().results()      # (the workspace now holds the first call's sums)
        bad = differences(case, first, want)
        assert not bad, "\n".join(bad)
        assert any(int(r.abs().max()) for r in first[:case.M]) and int(first[-1].abs().max())      # the case has gradients at all
        for a, b in zip(first, second):
            assert torch.equal(a, b), "two calls differ"
        B = case.shape[0]
        if B > 1:      # the batch in another order: the same table gradients, the planes of grad_x in that order
            perm = list(np.random.default_rng(B).permutation(B))
            if perm == list(range(B)):
                perm = perm[::-1]
            other = Call(case, perm=perm).run().results()
            for m in range(case.M):
                assert torch.equal(other[m], first[m]), "grad_wq[%d] depends on the order of the batch" % m
            assert torch.equal(other[-1], first[-1][perm]), "grad_x is not the same permutation of its planes"
    finally:
        case.free()


# ------------------------------------------------------------------------------------------------- 2. what is added, and to what
def test_zero_grad_out_writes_nothing_and_a_call_adds_to_what_is_there():
    case = fc.E7.build()
    rng = np.random.default_rng(77)
    prior = (rng.normal(0, 1e-4, case.tables.shape).astype(np.float32), rng.normal(0, 1e-4, case.shape).astype(np.float32))
    call = Call(case, prior=prior)
    before = call.results()
    kept = call.gout.clone()
    call.gout.zero_()
    after = call.run().results()
    for a, b in zip(before, after):
        assert torch.equal(a, b), "an all-zero grad_out changed a destination"
    call.gout.copy_(kept)
    got = call.run().results()
    want = fc.expected(case, prior=prior)
    bad = differences(case, got, want)
    assert not bad, "\n".join(bad)
    alone = fc.expected(case)
    assert np.array_equal(want.gx, prior[1] + alone.gx) and np.array_equal(want.gw, prior[0] + alone.gw)      # prior + value, one float add
    assert not np.array_equal(want.gx, alone.gx)
    case.free()


# ------------------------------------------------------------------------------------------------------------ 3. streams, capture
def test_call_on_a_non_blocking_side_stream():
    case = fc.CASES[0]
    want = fc.expected(case)
    call = Call(case)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()      # (torch's streams are non-blocking: no implicit order with the default stream)
    with torch.cuda.stream(side):
        call.run()
    side.synchronize()
    bad = differences(case, call.results(), want)
    case.free()
    assert not bad, "\n".join(bad)


def test_captured_call_replays_on_a_grad_out_rewritten_in_place():
    case = [c for c in fc.CASES if c.name.startswith("E2")][0].build()
    call = Call(case)
    call.run()                       # the warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.zero()
        call.run()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    bad = differences(case, call.results(), fc.expected(case))
    assert not bad, "\n".join(bad)
    new = torch.flip(call.gout, dims=[2, 3]) * 1.75      # another maximum: another scale
    call.gout.copy_(new)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    replayed = call.results()
    call.zero()
    direct = call.run().results()
    torch.cuda.synchronize()
    for a, b in zip(replayed, direct):
        assert torch.equal(a, b), "the replay differs from the direct call"
    case.gout = new.cpu().numpy()
    bad = differences(case, replayed, fc.expected(case))
    case.free()
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------------------------------------------------- 4. yardstick
def _shipped_tables(folder):
    from mulut_amd import load_lut_dict
    for key, t in load_lut_dict(os.path.join(GOLDEN, "luts"), 2, "sdy", 4, 4, "LUT_ft").items():
        np.save(os.path.join(str(folder), "LUT_x4_4bit_int8_%s.npy" % key), t)


def _grads(net, x, tgt):
    net.zero_grad()
    xg = x.clone().requires_grad_(True)
    torch.nn.functional.mse_loss(net(xg), tgt).backward()
    return [("grad_x", xg.grad)] + [(n, p.grad) for n, p in sorted(net.named_parameters())]


def _seeded_noise_tables(folder):
    """the tables of test_gpu_finetune.py::test_more_shapes_vs_cpu_oracle, the test whose natural crops ft_grad_bar.py's bar was set on"""
    for s in range(2):
        for m in "sdy":
            t = np.random.default_rng(3 * s + ord(m)).integers(-127, 128, size=(17 ** 4, 16 if s == 1 else 1), dtype=np.int8)
            np.save(os.path.join(str(folder), "LUT_x4_4bit_int8_s%d_%s.npy" % (s + 1, m)), t)


def test_fast_backward_against_the_exact_one_on_natural_crops(tmp_path):
    """8 natural-like 48 x 48 crops, 2-stage sdy x4 at interval 4: the float-atomic kernels are held to the fixed-point ones at the bar
    they are held to against the CPU oracle -- the reference side now computed on the device.
    Tables: those of test_more_shapes_vs_cpu_oracle, whose 'smooth' leg (these crops, 256 of them) is what the bar's element-wise part
    was measured on.  That part is a statement about such tables: an input-gradient term is (g . row_{j+1} - g . row_j) / q in float32,
    and on the SHIPPED tables neighbouring rows nearly cancel, so that the float32 expression itself -- in any order of its 16 products --
    sits 8.5e-5 element-wise from the float64 oracle (host model against oracle/ft_torch.py in float64 on two such crops, on the CPU;
    norm-wise 1.7e-6), above the bar before any kernel runs; on the seeded tables the same comparison gives 4.5e-6."""
    from mulut_amd.finetune import MuLUT
    from mulut_amd.synth import natural_frames
    _seeded_noise_tables(tmp_path)
    big = natural_frames(1, 270, 480, 1, 11)[0, :, :, 0]
    rng = np.random.default_rng(5)
    ys, xs = rng.integers(0, 270 - 48, 8), rng.integers(0, 480 - 48, 8)
    x = torch.from_numpy(np.stack([big[a:a + 48, b:b + 48] for a, b in zip(ys, xs)])[:, None].astype(np.float32) / np.float32(255)).cuda()
    tgt = torch.from_numpy(rng.random((8, 1, 192, 192), dtype=np.float32)).cuda()
    fast = _grads(MuLUT(str(tmp_path), 2, "sdy", upscale=4).cuda(), x, tgt)
    exact = _grads(MuLUT(str(tmp_path), 2, "sdy", upscale=4, deterministic=True).cuda(), x, tgt)
    for (name, g), (_, r) in zip(fast, exact):
        g, r = g.cpu().numpy(), r.cpu().numpy()
        scale = float(np.abs(r).max())
        assert scale > 0
        sig = np.abs(r) > 0.01 * scale
        print(name, "norm-wise %.3g element-wise %.3g" % (float(np.abs(g - r).max()) / scale, float((np.abs(g - r)[sig] / np.abs(r)[sig]).max())))
        ft_grad_bar.close(g, r, name)


# --------------------------------------------------------------------------------------------------------------- 5. module, driver
def test_module_backward_twice_gives_identical_gradient_bits(tmp_path):
    from mulut_amd.finetune import MuLUT
    _shipped_tables(tmp_path)
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.integers(0, 256, (4, 1, 24, 20)).astype(np.float32) / np.float32(255)).cuda()
    tgt = torch.from_numpy(rng.random((4, 1, 96, 80), dtype=np.float32)).cuda()
    net = MuLUT(str(tmp_path), 2, "sdy", upscale=4, deterministic=True).cuda()
    a = [(n, bits(g).clone()) for n, g in _grads(net, x, tgt)]
    b = [(n, bits(g).clone()) for n, g in _grads(net, x, tgt)]
    for (n, ga), (_, gb) in zip(a, b):
        assert int(ga.abs().max()) > 0, n
        assert torch.equal(ga, gb), n


def _train_dir(root):
    """three 96 x 96 pairs in the DIV2K layout: natural-like HR images and their 24 x 24 LR twins"""
    from PIL import Image
    from mulut_amd.synth import natural_frames
    os.makedirs(os.path.join(root, "HR"))
    os.makedirs(os.path.join(root, "LR", "X4"))
    for i, hr in enumerate(natural_frames(3, 96, 96, 3, 21)):
        Image.fromarray(hr).save(os.path.join(root, "HR", "%04d.png" % i))
        Image.fromarray(hr).resize((24, 24), Image.BICUBIC).save(os.path.join(root, "LR", "X4", "%04dx4.png" % i))
    return root


def _seeded_tables(exp, modes, interval):      # as tests/test_gpu_ft_wide.py: smooth ramp tables with seeded noise
    import reach_cases as rc
    for s in (1, 2):
        for i, m in enumerate(modes):
            t = rc.table("ramp", interval, 16 if s == 2 else 1, seed=10 * s + i, final=s == 2)
            np.save(os.path.join(exp, "LUT_x4_%dbit_int8_s%d_%s.npy" % (interval, s, m)), np.clip(t, -127, 127).astype(np.int8))


@pytest.mark.parametrize("modes,interval", [("sdy", 4), ("sdyeho", 5)])
def test_driver_twice_with_one_seed_gives_the_same_run(tmp_path, modes, interval):
    """8 iterations at batch 4 x crop 16 of --deterministic --seed 3, twice: the float parameters bit for bit, the exported tables, the
    LUT_ft files and the losses are the same."""
    from mulut_amd import finetune_lut
    train = _train_dir(str(tmp_path / "train"))
    runs = []
    for k in range(2):
        exp = str(tmp_path / ("exp%d" % k))
        os.makedirs(exp)
        _seeded_tables(exp, modes, interval)
        log = []
        opt = finetune_lut.build_parser().parse_args(["--stages", "2", "--modes", modes, "--interval", str(interval), "-e", exp, "--trainDir", train,
                                                      "--batchSize", "4", "--cropSize", "16", "--totalIter", "8", "--displayStep", "4", "--lr0", "1e-3",
                                                      "--seed", "3", "--deterministic", "--valDir", str(tmp_path / "none"), "--valStep", "1000"])
        run = finetune_lut.FinetuneRun(opt, log.append)
        for _ in range(8):
            run.step()
        losses = run.finish()
        assert sum("deterministic backward" in line for line in log) == 1
        files = {f: open(os.path.join(exp, f), "rb").read() for f in sorted(os.listdir(exp)) if f.startswith("LUT_ft_")}
        runs.append((losses, {n: bits(p.detach()).cpu() for n, p in run.net.named_parameters()}, run.net.export_int8(), files))
    (l0, p0, t0, f0), (l1, p1, t1, f1) = runs
    assert len(l0) == 8 and l0 == l1 and all(np.isfinite(l0))
    assert len(f0) == 2 * len(modes) and f0 == f1
    moved = 0
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
        moved += int((p0[n] != bits(torch.from_numpy(np.load(os.path.join(str(tmp_path / "exp0"), "LUT_x4_%dbit_int8_%s.npy" % (interval, n[len("weight_"):]))
                                                             ).astype(np.float32).reshape(p0[n].shape) / np.float32(127.0)))).sum())
    assert moved > 0      # the run trained something
    for k in t0:
        assert np.array_equal(t0[k], t1[k]), k
