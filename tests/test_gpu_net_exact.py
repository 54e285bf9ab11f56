"""The bit-reproducible backward of the SR network on the GPU (-m gpu): the gather kernel against the host model bit for bit, the exact
backward at op level (the gradient bar of tests/net_train_cases.py, gw / gb equal to the default backward's, gx equal from run to run
and for every workspace size, written and not added), the gradients of a two-stage model from run to run, the driver with
--deterministic twice, an exact resume with --saveOpt, and side streams / a captured graph."""
import copy
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

import net_cases as nc
import net_exact_cases as xc
import net_train_cases as tc

pytestmark = pytest.mark.gpu


def _bits(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)


@pytest.fixture(scope="module")
def trainers():
    from mulut_amd.net_train import NetTrainer
    made = {name: NetTrainer(tc.model(name).cuda(), deterministic=True) for name in tc.MODELS}
    yield made
    for t in made.values():
        t.close()


def _raw_backward(tr, stage, x, g, gx, ws, grads):
    """mulut_net_stage_backward_exact into the caller's buffers, on the current stream."""
    M = len(tr.modes)
    N, C, H, W = x.shape
    gw = (ctypes.c_void_p * (6 * M))(*[grads[12 * m + l].data_ptr() for m in range(M) for l in range(6)])
    gb = (ctypes.c_void_p * (6 * M))(*[grads[12 * m + 6 + l].data_ptr() for m in range(M) for l in range(6)])
    rc = tr._lib.mulut_net_stage_backward_exact(tr._handles(stage), tr.modes.encode(), x.data_ptr(), g.data_ptr(), N, C, H, W, ws.data_ptr(), ws.numel(),
                                                gx.data_ptr(), gw, gb, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc


# ------------------------------------------------------------------------------------------------- 1. the gather against the host model
@pytest.mark.parametrize("shape", xc.OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_is_the_host_model_bit_for_bit(trainers, shape):
    """Every pattern letter, r 0..3, ts exact and with 128 of slack (filled with NaN: never read), written into a NaN-filled gx; then
    all 24 passes of "sdyeho" chained, the first written and the others added.  t is standard normal times 2^(-20..20) per element,
    so another order of a pixel's adds shows in the last bits."""
    tr = trainers["tiny"]
    total = int(np.prod(shape))
    rng = np.random.default_rng([11] + list(shape))
    for slack in (0, 128):
        ts = total + slack
        t = xc.mixed_taps(rng, 24, ts)
        t[:, :, total:] = np.nan
        td = torch.from_numpy(t).cuda()
        chain = None
        for mi, mode in enumerate(xc.LETTERS):
            for r in range(4):
                p = 4 * mi + r
                got = tr.gx_gather(mode, r, td[p], shape)
                want = xc.host_pass(mode, r, t[p], shape)
                assert np.isfinite(want).all() and np.array_equal(_bits(got), _bits(want)), (mode, r, shape, ts)
                chain = got.clone() if chain is None else tr.gx_gather(mode, r, td[p], shape, gx=chain)
        want = xc.host_stage(xc.LETTERS, t, shape)
        assert np.array_equal(_bits(chain), _bits(want)), (shape, ts)


# ------------------------------------------------------------------------------------------------------------------- 2. op level
@pytest.mark.parametrize("cfg", xc.OP_MODELS, ids=xc.model_id)
def test_exact_backward_at_op_level(cfg):
    """Every shape and stage.  gx meets the bar the default path is held to (another order over sums of the same length and type);
    gw / gb are the default backward's bits; gx is the same bits over two runs and between the default workspace and the smallest
    one; a NaN-filled gx comes back finite; gx = NULL gives the same gw / gb."""
    from mulut_amd.net_train import NetTrainer
    net = nc.seeded_model(**cfg)
    tr, plain = NetTrainer(copy.deepcopy(net).cuda(), deterministic=True), NetTrainer(copy.deepcopy(net).cuda())
    worst = 0.0
    for shape in xc.OP_SHAPES:
        for s in range(1, cfg["stages"] + 1):
            case = xc.op_case(cfg, shape, s, "cuda")
            x, g = case["x"], case["g"]
            what = "%s %r s%d" % (xc.model_id(cfg), shape, s)
            tr.load(s)
            plain.load(s)
            gx, gp = tr._backward(s, x, g, True)
            gx_again, gp_again = tr._backward(s, x, g, True)
            small = tr.workspace(s, x.numel(), min_sites=128)
            assert small.numel() == tr._lib.mulut_net_backward_exact_ws_bytes(cfg["nf"], case["u"], 128, x.numel())
            gx_small, gp_small = tr._backward(s, x, g, True, ws=small)
            none, gp_none = tr._backward(s, x, g, False)
            _, gp_plain = plain._backward(s, x, g, True)
            assert none is None
            worst = max(worst, xc.meets(gx, case["gx64"], what + " gx"))
            assert torch.equal(gx, gx_again) and torch.equal(gx, gx_small), what
            for a, b, c, d, e in zip(gp, gp_again, gp_small, gp_none, gp_plain):
                assert torch.equal(a, b) and torch.equal(a, d) and torch.equal(a, e), what
            pn = {id(p): n for n, p in tr.model.named_parameters()}
            for p, c in zip(tr.stage_params(s), gp_small):      # (the smallest workspace splits the weight-gradient sums otherwise: the bar, as for the default path)
                worst = max(worst, xc.meets(c, case["gp64"][pn[id(p)]], what + " " + pn[id(p)] + " (smallest workspace)"))
            filled = torch.full_like(x, float("nan"))
            grads = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in tr.stage_params(s)]
            _raw_backward(tr, s, x, g, filled, tr.workspace(s, x.numel()), grads)
            assert torch.isfinite(filled).all() and torch.equal(filled, gx), what
    print("%s: largest distance %.3g (bar %.3g)" % (xc.model_id(cfg), worst, xc.C))
    tr.close()
    plain.close()


# ------------------------------------------------------------------------------------------------ 3. gradients through two stages
def test_gradients_through_two_stages_are_the_same_bits(trainers):
    fx, cfg, tr = tc.fixture(), tc.MODELS["sd2"], trainers["sd2"]
    S = cfg["stages"]
    net64 = copy.deepcopy(tr.model).double()
    for c in tc.cases("sd2"):
        key = "sd2/%s" % c
        x = torch.from_numpy(fx[key + "/x"].astype(np.float32) / 255.0).cuda()
        lb = torch.from_numpy(fx[key + "/lb"].astype(np.float32) / 255.0).cuda()
        runs = []
        for _ in range(2):
            tr.model.zero_grad()
            tr.keep_sums = True
            loss = F.mse_loss(tr.predict(x, "train"), lb)
            loss.backward()
            sums = [tr.last_sums[s].detach().clone() for s in range(1, S + 1)]
            tr.keep_sums, tr.last_sums = False, {}
            runs.append((loss.item(), {n: p.grad.detach().clone() for n, p in tr.model.named_parameters()}))
        assert runs[0][0] == runs[1][0]
        for n in runs[0][1]:
            assert torch.equal(runs[0][1][n], runs[1][1][n]), (key, n)
        net64.zero_grad()
        out64, _ = tc.predict_train(net64, x.double(), cfg["modes"], S, forced=[t.double() for t in sums])
        F.mse_loss(out64, lb.double()).backward()
        for n, p in net64.named_parameters():
            tc.meets(runs[1][1][n], p.grad, "%s %s" % (key, n))


# ------------------------------------------------------------------------------------------------------------------- 4. the driver
@pytest.fixture(scope="module")
def bench_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("bench")
    shutil.copytree(os.path.join(GOLDEN, "Set5", "HR"), str(root / "Set5" / "HR"))
    shutil.copytree(os.path.join(GOLDEN, "Set5", "LR_bicubic"), str(root / "Set5" / "LR_bicubic"))
    return str(root)


def _drive(exp, bench, extra=()):
    """The 12-iteration configuration of tests/test_gpu_net_train.py; a flag given again in `extra` overrides it."""
    from mulut_amd import train_model
    from mulut_amd.options import TrainOptions
    opt = TrainOptions().parse(["-e", str(exp), "--nf", "8", "--stages", "2", "--modes", "sd", "--scale", "4", "--batchSize", "4", "--cropSize", "12",
                                "--trainDir", os.path.join(GOLDEN, "Set5"), "--valDir", bench, "--totalIter", "12", "--displayStep", "1",
                                "--saveStep", "12", "--valStep", "12", "--seed", "3"] + list(extra))
    lines = []
    model_G, losses = train_model.train(opt, lines.append)
    return opt, lines, model_G, losses


def _tensors(path):
    from mulut_amd import network
    return {k: v.cpu() for k, v in network.load_checkpoint(path).state_dict().items()}


def test_driver_twice_writes_the_same_checkpoint(tmp_path, bench_dir):
    runs = [_drive(tmp_path / name, bench_dir, ["--deterministic"]) for name in ("a", "b")]
    (_, lines_a, _, losses_a), (_, lines_b, _, losses_b) = runs
    assert len(losses_a) == 12 and losses_a == losses_b
    a, b = _tensors(str(tmp_path / "a" / "Model_000012.pth")), _tensors(str(tmp_path / "b" / "Model_000012.pth"))
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    det = [ln for ln in lines_a if "deterministic backward" in ln]
    assert len(det) == 1 and "no --seed" not in det[0]
    assert [ln for ln in lines_a if "AVG Val PSNR" in ln] == [ln for ln in lines_b if "AVG Val PSNR" in ln]
    assert not os.path.exists(str(tmp_path / "a" / "Opt_000012.pth"))      # --saveOpt is off


def test_driver_without_a_seed_says_so(tmp_path):
    from mulut_amd import train_model
    from mulut_amd.options import TrainOptions
    opt = TrainOptions().parse(["-e", str(tmp_path / "e"), "--nf", "8", "--stages", "2", "--modes", "sd", "--scale", "4", "--batchSize", "4", "--cropSize", "12",
                                "--trainDir", os.path.join(GOLDEN, "Set5"), "--valDir", str(tmp_path / "none"), "--totalIter", "1", "--displayStep", "1",
                                "--saveStep", "100", "--valStep", "100", "--deterministic"])
    lines = []
    train_model.train(opt, lines.append)
    det = [ln for ln in lines if "deterministic backward" in ln]
    assert len(det) == 1 and "no --seed" in det[0]


# ------------------------------------------------------------------------------------------------------------------- 5. the resume
def test_resume_with_the_optimiser_state_is_exact(tmp_path, bench_dir):
    """Straight through to 12 against --startIter 8 from the files of iteration 8.  (--saveStep 4, not 8: Model_000012.pth, which is
    compared, is only written by a step that divides 12; iteration 8 is saved either way.)"""
    none = str(tmp_path / "none")
    common = ["--deterministic", "--saveOpt", "--saveStep", "4", "--totalIter", "12", "--valStep", "100"]
    _, lines_s, _, losses_s = _drive(tmp_path / "straight", none, common)
    straight = str(tmp_path / "straight")
    assert all(os.path.exists(os.path.join(straight, "%s_%06d.pth" % (k, i))) for k in ("Model", "Opt") for i in (4, 8, 12))
    assert not any("optimiser state loaded" in ln for ln in lines_s)
    for name, files in (("resumed", ("Model_000008.pth", "Opt_000008.pth")), ("fresh", ("Model_000008.pth",))):
        os.makedirs(str(tmp_path / name))
        for f in files:
            shutil.copy(os.path.join(straight, f), str(tmp_path / name / f))
    _, lines_r, _, losses_r = _drive(tmp_path / "resumed", none, common + ["--startIter", "8"])
    assert len(losses_r) == 4 and losses_r == losses_s[8:]
    a, b = _tensors(os.path.join(straight, "Model_000012.pth")), _tensors(str(tmp_path / "resumed" / "Model_000012.pth"))
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert len([ln for ln in lines_r if "optimiser state loaded" in ln]) == 1
    # and the state the next resume would load is the straight run's, too
    oa = torch.load(os.path.join(straight, "Opt_000012.pth"), map_location="cpu", weights_only=False)
    ob = torch.load(str(tmp_path / "resumed" / "Opt_000012.pth"), map_location="cpu", weights_only=False)
    assert oa["rng"] == ob["rng"] and oa["opt_G"]["param_groups"] == ob["opt_G"]["param_groups"]
    for k, st in oa["opt_G"]["state"].items():
        assert all(torch.equal(st[n], ob["opt_G"]["state"][k][n]) for n in st), k
    # without Opt_000008.pth: today's resume, no such line, a fresh optimiser and so another trajectory
    _, lines_f, _, losses_f = _drive(tmp_path / "fresh", none, common + ["--startIter", "8"])
    assert not any("optimiser state loaded" in ln for ln in lines_f) and len(losses_f) == 4 and losses_f != losses_s[8:]


# ---------------------------------------------------------------------------------------------------- 6. streams and graphs
def test_side_stream_and_captured_graph(trainers):
    tr = trainers["sd2"]
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.integers(0, 256, (2, 1, 33, 17), dtype=np.uint8).astype(np.float32) / 255.0).cuda()
    g = torch.from_numpy(rng.standard_normal((2, 1, 66, 34)).astype(np.float32)).cuda()
    tr.load(2)
    want_gx, want_gp = tr._backward(2, x, g, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got_gx, got_gp = tr._backward(2, x, g, True)
    side.synchronize()
    assert torch.equal(got_gx, want_gx) and all(torch.equal(a, b) for a, b in zip(got_gp, want_gp))
    # a captured backward (a linear chain) replays on rewritten inputs
    ws = tr.workspace(2, x.numel())
    gx = torch.full_like(x, float("nan"))
    grads = [torch.zeros_like(p) for p in tr.stage_params(2)]
    _raw_backward(tr, 2, x, g, gx, ws, grads)      # the warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _raw_backward(tr, 2, x, g, gx, ws, grads)
    torch.cuda.synchronize()
    gx.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gx, want_gx) and all(torch.equal(a, b) for a, b in zip(grads, want_gp))
    x.copy_(torch.from_numpy(rng.integers(0, 256, (2, 1, 33, 17), dtype=np.uint8).astype(np.float32) / 255.0))
    g.copy_(torch.from_numpy(rng.standard_normal((2, 1, 66, 34)).astype(np.float32)))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    direct_gx, direct_gp = tr._backward(2, x, g, True)
    assert torch.equal(gx, direct_gx) and not torch.equal(gx, want_gx)
    assert all(torch.equal(a, b) for a, b in zip(grads, direct_gp))
