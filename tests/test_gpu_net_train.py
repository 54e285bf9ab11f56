"""Training the network on the GPU (-m gpu): the device pack of both weight streams against the host packs bit for bit, the 'train'-phase
stage forward against the reference-made fixtures and the pass form, the backward against a float64 restatement on the same inputs,
`NetTrainer.predict` + loss + `.backward()` end to end on the fixture batches, the driver, and side streams / a captured graph.

The gradient bar, the kink-free g and where both come from: tests/net_train_cases.py."""
import copy
import ctypes
import os
import re
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

import net_cases as nc
import net_train_cases as tc

pytestmark = pytest.mark.gpu


def _lib():
    from mulut_amd import _native
    return _native.load()


def _random_unit(nf, u, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.standard_normal((nf if l < 5 else u * u, 4 if l == 0 else l * nf)).astype(np.float32) for l in range(6)]
    bs = [rng.standard_normal(nf if l < 5 else u * u).astype(np.float32) for l in range(6)]
    return ws, bs


# ---------------------------------------------------------------------------------------------------------------- 1. device pack
@pytest.mark.parametrize("nf", [8, 24, 33, 64])
def test_device_pack_is_the_host_pack_bit_for_bit(nf):
    lib = _lib()
    fp = ctypes.POINTER(ctypes.c_float)
    for u in (1, 2, 3, 4):
        ws, bs = _random_unit(nf, u, 100 * nf + u)
        wp, bp = (fp * 6)(*[w.ctypes.data_as(fp) for w in ws]), (fp * 6)(*[b.ctypes.data_as(fp) for b in bs])
        dw, db = [torch.from_numpy(w).cuda() for w in ws], [torch.from_numpy(b).cuda() for b in bs]
        h = ctypes.c_void_p()
        assert lib.mulut_net_unit_create_train(0, nf, u, ctypes.byref(h)) == 0
        try:
            assert lib.mulut_net_unit_load_dev(h, (ctypes.c_void_p * 6)(*[t.data_ptr() for t in dw]), (ctypes.c_void_p * 6)(*[t.data_ptr() for t in db]),
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            for backward in (0, 1):
                host = np.full(1 << 18, np.nan, np.float32)
                n = lib.mulut_net_pack_host(nf, u, wp, bp, backward, host.ctypes.data, host.size)
                assert n > 0 and n % 4096 == 0
                dev = np.full(n, np.nan, np.float32)
                assert lib.mulut_net_unit_read(h, backward, dev.ctypes.data, n) == n
                assert np.array_equal(dev.view(np.uint32), host[:n].view(np.uint32)), (nf, u, backward)
                assert np.count_nonzero(dev) > 0
        finally:
            lib.mulut_net_unit_destroy(h)


def test_load_weights_gives_the_tables_of_a_fresh_engine():
    from mulut_amd.net_engine import NetEngine
    net = nc.seeded_model(nf=24, scale=2, modes="sy", stages=2, seed=7)
    eng = NetEngine(net)
    before = eng.table(2, "y", 6)
    moved = copy.deepcopy(net).cuda()
    with torch.no_grad():
        for p in moved.parameters():
            p.mul_(0.9).add_(0.01)
    eng.load_weights(moved)
    fresh = NetEngine(moved.cpu())
    for s in (1, 2):
        for m in "sy":
            assert torch.equal(eng.table(s, m, 6), fresh.table(s, m, 6)), (s, m)
    assert not torch.equal(eng.table(2, "y", 6), before)
    eng.close()
    fresh.close()


# --------------------------------------------------------------------------------------------------------- 2. stage_sum forward
def _sum_bar(got, want, M, what):
    worst, share = nc.off(got, want)
    print("%s: worst %d, share off %.3g of %d (caps %d, %.3g)" % (what, worst, share, np.asarray(want).size, 4 * M, 4 * M * nc.BAR))
    assert worst <= 4 * M and share <= 4 * M * nc.BAR, (what, worst, share)


@pytest.fixture(scope="module")
def trainers():
    from mulut_amd.net_train import NetTrainer
    made = {name: NetTrainer(tc.model(name).cuda()) for name in tc.MODELS}
    yield made
    for t in made.values():
        t.close()


def test_stage_sum_against_the_fixture_sums(trainers):
    fx = tc.fixture()
    for name, cfg in tc.MODELS.items():
        tr, M = trainers[name], len(cfg["modes"])
        got, want = [], []
        for c in tc.cases(name):
            x = torch.from_numpy(fx["%s/%s/x" % (name, c)].astype(np.float32) / 255.0).cuda()
            for s in range(1, cfg["stages"] + 1):
                with torch.no_grad():
                    p = tr.stage_sum(s, x)
                    again = tr.stage_sum(s, x)
                assert torch.equal(p, again) and torch.equal(p, torch.round(p))
                ref = torch.from_numpy(fx["%s/%s/s%d/sum" % (name, c, s)].astype(np.float32)).cuda()
                got.append(p.cpu().numpy().astype(np.int32).ravel())
                want.append(ref.cpu().numpy().astype(np.int32).ravel())
                x = tc.round_func(torch.clamp(ref / (M * 4) + 127, 0, 255)) / 255.0      # the next stage on the reference's input
        _sum_bar(np.concatenate(got), np.concatenate(want), M, name + " sums")


@pytest.mark.parametrize("cfg", tc.OP_MODELS, ids=tc.model_id)
def test_stage_sum_is_the_sum_of_the_pass_form(cfg):
    from mulut_amd.net_engine import NetEngine
    from mulut_amd.net_train import NetTrainer
    net = nc.seeded_model(**cfg)
    eng, tr = NetEngine(net), NetTrainer(copy.deepcopy(net).cuda())
    rng = np.random.default_rng(cfg["seed"])
    got, want = [], []
    for shape in tc.OP_SHAPES:
        xb = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).cuda()
        for s in range(1, cfg["stages"] + 1):
            with torch.no_grad():
                p = tr.stage_sum(s, xb.float() / 255.0)
            ref = torch.stack([eng.pass_(s, m, r, xb) for m in cfg["modes"] for r in range(4)]).to(torch.int32).sum(0)
            got.append(p.cpu().numpy().astype(np.int32).ravel())
            want.append(ref.cpu().numpy().ravel())
    _sum_bar(np.concatenate(got), np.concatenate(want), len(cfg["modes"]), tc.model_id(cfg) + " sums against passes")
    eng.close()
    tr.close()


# -------------------------------------------------------------------------------------------------------- 3. op-level backward
@pytest.mark.parametrize("cfg", tc.OP_MODELS, ids=tc.model_id)
def test_backward_against_float64_on_the_same_inputs(cfg):
    """Every shape and stage, with the default workspace and with the smallest one (one workgroup's sites: the chunk loop and the
    partial accumulation run once per 128 sites); gx = NULL gives the same gw; two runs give the same gw / gb bits."""
    from mulut_amd.net_train import NetTrainer
    tr = NetTrainer(copy.deepcopy(nc.seeded_model(**cfg)).cuda())
    names = None
    worst = 0.0
    for shape in tc.OP_SHAPES:
        for s in range(1, cfg["stages"] + 1):
            case = tc.op_case(cfg, shape, s, "cuda")
            assert case["dropped"] <= tc.MAX_DROP
            x, g = case["x"], case["g"]
            if names is None or s != names[0]:
                pn = {id(p): n for n, p in tr.model.named_parameters()}
                names = (s, [pn[id(p)] for p in tr.stage_params(s)])
            tr.load(s)
            what = "%s %r s%d" % (tc.model_id(cfg), shape, s)
            gx, gp = tr._backward(s, x, g, True)
            small = tr.workspace(s, 128, min_sites=128)
            gx_small, gp_small = tr._backward(s, x, g, True, ws=small)
            none, gp_none = tr._backward(s, x, g, False)
            _, gp_again = tr._backward(s, x, g, True)
            assert none is None
            for n, a, b, c, d in zip(names[1], gp, gp_small, gp_none, gp_again):
                assert torch.equal(a, c) and torch.equal(a, d), (what, n)
                worst = max(worst, tc.meets(a, case["gp64"][n], what + " " + n), tc.meets(b, case["gp64"][n], what + " " + n + " (smallest workspace)"))
            worst = max(worst, tc.meets(gx, case["gx64"], what + " gx"), tc.meets(gx_small, case["gx64"], what + " gx (smallest workspace)"))
    print("%s: largest distance %.3g (bar %.3g)" % (tc.model_id(cfg), worst, tc.C))
    tr.close()


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("name", sorted(tc.MODELS))
def test_predict_loss_and_backward_on_the_fixture_batches(trainers, name):
    fx, cfg, tr = tc.fixture(), tc.MODELS[name], trainers[name]
    M, S = len(cfg["modes"]), cfg["stages"]
    net64 = copy.deepcopy(tr.model).double()
    for c in tc.cases(name):
        key = "%s/%s" % (name, c)
        x = torch.from_numpy(fx[key + "/x"].astype(np.float32) / 255.0).cuda()
        lb = torch.from_numpy(fx[key + "/lb"].astype(np.float32) / 255.0).cuda()
        tr.model.zero_grad()
        tr.keep_sums = True
        loss = F.mse_loss(tr.predict(x, "train"), lb)
        loss.backward()
        sums = [tr.last_sums[s].detach().clone() for s in range(1, S + 1)]
        tr.keep_sums, tr.last_sums = False, {}
        for s in range(S):      # (every stage ran on the trainer's own cascade; the fixture's case has the same integers in float32 and float64)
            _sum_bar(sums[s].cpu().numpy().astype(np.int32), fx["%s/s%d/sum" % (key, s + 1)].astype(np.int32), M, "%s s%d sums" % (key, s + 1))
        net64.zero_grad()
        out64, _ = tc.predict_train(net64, x.double(), cfg["modes"], S, forced=[t.double() for t in sums])
        loss64 = F.mse_loss(out64, lb.double())
        loss64.backward()
        print("%s: loss %.9g, restatement %.17g, reference %.17g" % (key, loss.item(), loss64.item(), float(fx[key + "/loss64"])))
        assert abs(loss.item() - loss64.item()) <= tc.LOSS_RTOL * abs(loss64.item())
        got = dict(tr.model.named_parameters())
        for n, p in net64.named_parameters():
            tc.meets(got[n].grad, p.grad, "%s %s" % (key, n))


# ------------------------------------------------------------------------------------------------------------------- 5. the driver
@pytest.fixture(scope="module")
def bench_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("bench")
    shutil.copytree(os.path.join(GOLDEN, "Set5", "HR"), str(root / "Set5" / "HR"))
    shutil.copytree(os.path.join(GOLDEN, "Set5", "LR_bicubic"), str(root / "Set5" / "LR_bicubic"))
    return str(root)


def _drive(exp, bench, extra=()):
    from mulut_amd import train_model
    from mulut_amd.options import TrainOptions
    opt = TrainOptions().parse(["-e", str(exp), "--nf", "8", "--stages", "2", "--modes", "sd", "--scale", "4", "--batchSize", "4", "--cropSize", "12",
                                "--trainDir", os.path.join(GOLDEN, "Set5"), "--valDir", bench, "--totalIter", "12", "--displayStep", "1",
                                "--saveStep", "12", "--valStep", "12", "--seed", "3"] + list(extra))
    lines = []
    model_G, losses = train_model.train(opt, lines.append)
    return opt, lines, model_G, losses


def test_driver_runs_saves_validates_and_transfers(tmp_path, bench_dir):
    from mulut_amd import network, transfer_to_lut as T
    from mulut_amd.net_engine import NetEngine
    from mulut_amd.net_val import net_valid_steps
    exp = tmp_path / "exp"
    opt, lines, model_G, losses = _drive(exp, bench_dir)
    shown = [ln for ln in lines if "GPixel" in ln]
    assert len(shown) == 12 and len(losses) == 12 and all(np.isfinite(losses))
    pat = re.compile(re.escape(str(exp)) + r" \| Iter: {4,5}\d{1,2}, Sample: {4,5}\d{1,2}, GPixel:\d\.\d\de[-+]\d\d, dT:\d+\.\d{4}, rT:\d+\.\d{4}$")
    assert all(pat.match(ln) for ln in shown), shown[0]
    assert "Checkpoint saved 12" in lines and lines[-1] == "Complete"
    val = [ln for ln in lines if "AVG Val PSNR" in ln]
    assert len(val) == 1 and val[0].startswith("Iter 12 | Dataset Set5 | AVG Val PSNR: ")
    ckpt = os.path.join(str(exp), "Model_000012.pth")
    loaded = network.load_checkpoint(ckpt)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(model_G.state_dict().values(), loaded.state_dict().values()))
    eng = NetEngine(loaded)
    again = []
    net_valid_steps(eng, SimpleNamespace(valDir=bench_dir, valoutDir=str(tmp_path / "val2"), scale=4, debug=True), 12, again.append)
    assert again == val
    tabs = T.main(["--stages", "2", "--modes", "sd", "--scale", "4", "--nf", "8", "-e", str(exp), "--loadIter", "12", "--fused"])
    assert sorted(tabs) == ["s1_d", "s1_s", "s2_d", "s2_s"] and tabs["s2_s"].shape == (83521, 1, 4, 4)
    assert np.array_equal(tabs["s2_d"], eng.table(2, "d", 4).cpu().numpy())
    eng.close()
    # the torch path from the same seed: the same weights and crops, so the same first loss
    _, lines_t, _, losses_t = _drive(tmp_path / "exp_torch", bench_dir, ["--torchPath"])
    first = float(re.search(r"GPixel:(\S+),", shown[0]).group(1)), float(re.search(r"GPixel:(\S+),", [ln for ln in lines_t if "GPixel" in ln][0]).group(1))
    print("first GPixel: fused %r torch %r; losses %r / %r" % (first[0], first[1], losses[:3], losses_t[:3]))
    assert abs(losses[0] - losses_t[0]) <= 1e-5 * abs(losses_t[0]) and first[0] == first[1]


def test_driver_resumes_from_a_checkpoint(tmp_path, bench_dir):
    """--startIter N: the parameters of Model_{N:06d}.pth, the schedule advanced to N, the iteration count going on from N + 1."""
    import math
    from mulut_amd import network, train_model
    from mulut_amd.options import TrainOptions
    exp = tmp_path / "exp"
    opt, lines, model_G, losses = _drive(exp, bench_dir)
    assert opt.lrTrace[0] == 1e-3 and len(opt.lrTrace) == 12
    saved = network.load_checkpoint(os.path.join(str(exp), "Model_000012.pth")).state_dict()
    common = ["-e", str(exp), "--nf", "8", "--stages", "2", "--modes", "sd", "--scale", "4", "--batchSize", "4", "--cropSize", "12",
              "--trainDir", os.path.join(GOLDEN, "Set5"), "--valDir", str(tmp_path / "none"), "--displayStep", "1", "--saveStep", "100",
              "--valStep", "100", "--seed", "3", "--startIter", "12"]
    # nothing left to run: the module is the checkpoint's
    opt0 = TrainOptions().parse(common + ["--totalIter", "12"])
    lines0 = []
    model0, losses0 = train_model.train(opt0, lines0.append)
    assert losses0 == [] and all(torch.equal(a.cpu(), b) for a, b in zip(model0.state_dict().values(), saved.values()))
    assert any("validation is skipped" in ln for ln in lines0)
    # four more iterations of a 16-iteration schedule: it stands at 12
    opt1 = TrainOptions().parse(common + ["--totalIter", "16"])
    lines1 = []
    _, losses1 = train_model.train(opt1, lines1.append)
    shown = [ln for ln in lines1 if "GPixel" in ln]
    assert len(losses1) == 4 and len(shown) == 4 and "Iter:    13, Sample:     4," in shown[0] and "Iter:    16," in shown[-1]
    want = [1e-3 * (((1 + math.cos(k * math.pi / 16)) / 2) * 0.9 + 0.1) for k in (12, 13, 14, 15)]
    assert np.allclose(opt1.lrTrace, want, rtol=1e-12, atol=0), (opt1.lrTrace, want)
    assert not any("AVG Val PSNR" in ln for ln in lines1)


def test_backward_after_a_parameter_write_is_an_error(trainers):
    tr = trainers["tiny"]
    x = torch.rand((1, 1, 5, 7), device="cuda")
    loss = tr.stage_sum(1, x).sum()
    with torch.no_grad():
        tr.stage_params(1)[0].mul_(1.0)      # an in-place write, as an optimiser step makes
    with pytest.raises(RuntimeError, match="changed between stage_sum and its backward"):
        loss.backward()
    tr.stage_sum(1, x).sum().backward()      # and a fresh forward / backward pair is fine
    tr.model.zero_grad()


def test_driver_refuses_more_than_one_gpu(tmp_path):
    from mulut_amd import train_model
    from mulut_amd.options import TrainOptions
    opt = TrainOptions().parse(["-e", str(tmp_path / "e"), "--gpuNum", "2"])
    with pytest.raises(SystemExit, match="one GPU"):
        train_model.train(opt, lambda s: None)


# ---------------------------------------------------------------------------------------------------- 6. streams and graphs
def test_side_stream_and_captured_graph(trainers):
    tr, cfg = trainers["sd2"], tc.MODELS["sd2"]
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.integers(0, 256, (2, 1, 33, 17), dtype=np.uint8).astype(np.float32) / 255.0).cuda()
    g = torch.from_numpy(rng.standard_normal((2, 1, 66, 34)).astype(np.float32)).cuda()
    with torch.no_grad():
        want_p = tr.stage_sum(2, x)
    want_gx, want_gp = tr._backward(2, x, g, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.no_grad():
            got_p = tr.stage_sum(2, x)
        got_gx, got_gp = tr._backward(2, x, g, True)
    side.synchronize()
    assert torch.equal(got_p, want_p) and all(torch.equal(a, b) for a, b in zip(got_gp, want_gp))
    tc.meets(got_gx, want_gx.double(), "gx on a side stream")      # (float atomics: the order of a pixel's terms is free)
    # a captured stage_sum + backward replays on a rewritten input
    lib, handles, ws = tr._lib, tr._handles(2), tr.workspace(2, x.numel())
    pred, gx = torch.zeros_like(want_p), torch.zeros_like(x)
    grads = [torch.zeros_like(p) for p in tr.stage_params(2)]
    M = len(cfg["modes"])
    gw = (ctypes.c_void_p * (6 * M))(*[grads[12 * m + l].data_ptr() for m in range(M) for l in range(6)])
    gb = (ctypes.c_void_p * (6 * M))(*[grads[12 * m + 6 + l].data_ptr() for m in range(M) for l in range(6)])

    def both():
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.mulut_net_stage_sum(handles, b"sd", x.data_ptr(), 2, 1, 33, 17, pred.data_ptr(), st) == 0
        gx.zero_()
        assert lib.mulut_net_stage_backward(handles, b"sd", x.data_ptr(), g.data_ptr(), 2, 1, 33, 17, ws.data_ptr(), ws.numel(), gx.data_ptr(), gw, gb, st) == 0
    both()      # the warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pred, want_p) and all(torch.equal(a, b) for a, b in zip(grads, want_gp))
    x.copy_(torch.from_numpy(rng.integers(0, 256, (2, 1, 33, 17), dtype=np.uint8).astype(np.float32) / 255.0))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        direct_p = tr.stage_sum(2, x)
    _, direct_gp = tr._backward(2, x, g, True)
    assert torch.equal(pred, direct_p) and not torch.equal(pred, want_p)
    assert all(torch.equal(a, b) for a, b in zip(grads, direct_gp))
