"""Training the network without a GPU: what tests/golden/net_train_fixtures.npz (gen_golden_net_train.py: the reference's own
mulut_predict(..., 'train'), mse_loss and backward) holds, the torch restatement of tests/net_train_cases.py against it, the float32
distance the gradient bar is built on, the host half of the training entry points as a program of its own under sanitizers, the
backward-stream pack through the library against plain transposed matrices, and the command line."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT

import net_cases as nc
import net_train_cases as tc


def test_the_fixture_holds_what_it_claims():
    fx = tc.fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "net_train_fixtures.npz")) < (1 << 20)
    for name, cfg in tc.MODELS.items():
        assert tc.cases(name) == ["2x5x7", "4x12x12"]
        M, u = len(cfg["modes"]), cfg["scale"]
        for c in tc.cases(name):
            key = "%s/%s" % (name, c)
            x, lb = fx[key + "/x"], fx[key + "/lb"]
            N, C, H, W = x.shape
            assert x.dtype == np.uint8 and lb.dtype == np.uint8 and C == 1 and lb.shape == (N, 1, H * u, W * u)
            for s in range(1, cfg["stages"] + 1):
                p = fx["%s/s%d/sum" % (key, s)]
                us = u if s == cfg["stages"] else 1
                assert p.dtype == np.int16 and p.shape == (N, 1, H * us, W * us) and np.abs(p).max() <= 127 * 4 * M
            # the generator kept the case because nothing sits on a kink: the real g of the loss can be used as it is.  Recomputed
            # here as the generator computes it (float64, every stage on the float64 run's own input), not taken on trust
            net64 = tc.model(name).double()
            xs, mp = torch.from_numpy(x.astype(np.float32) / 255.0).double(), np.inf
            with torch.no_grad():
                _, stage_sums = tc.predict_train(net64, xs, cfg["modes"], cfg["stages"])
            for s in range(1, cfg["stages"] + 1):
                if s > 1:
                    xs = tc.round_func(torch.clamp(stage_sums[s - 2] / (M * 4) + 127, 0, 255)) / 255.0
                mp = min(mp, float(tc.min_preact(net64, xs, cfg["modes"], s).min()))
            print("%s: smallest |pre-activation| %.3g (fixture %.3g)" % (key, mp, float(fx[key + "/min_preact"])))
            assert mp >= 1e-6 and mp == float(fx[key + "/min_preact"])
            assert abs(float(fx[key + "/loss"]) - float(fx[key + "/loss64"])) <= 1e-6 * float(fx[key + "/loss64"])
            names = [n for n, _ in tc.model(name).named_parameters()]
            assert all("%s/grad/%s" % (key, n) in fx and fx["%s/grad64/%s" % (key, n)].dtype == np.float64 for n in names)


def test_restatement_is_the_reference_on_the_fixture_batches():
    """Sums equal; loss and every gradient within the bar of the reference's float64 run -- in float32 and in float64."""
    fx = tc.fixture()
    worst = 0.0
    for name, cfg in tc.MODELS.items():
        for dtype in (torch.float32, torch.float64):
            net = tc.model(name).to(dtype)
            for c in tc.cases(name):
                key = "%s/%s" % (name, c)
                x = torch.from_numpy(fx[key + "/x"].astype(np.float32) / 255.0).to(dtype)
                lb = torch.from_numpy(fx[key + "/lb"].astype(np.float32) / 255.0).to(dtype)
                net.zero_grad()
                out, sums = tc.predict_train(net, x, cfg["modes"], cfg["stages"])
                loss = F.mse_loss(out, lb)
                loss.backward()
                for s, p in enumerate(sums, 1):
                    assert np.array_equal(p.detach().numpy().astype(np.int16), fx["%s/s%d/sum" % (key, s)]), (key, s)
                assert abs(loss.item() - float(fx[key + "/loss64"])) <= tc.LOSS_RTOL * float(fx[key + "/loss64"])
                # forcing the sums it already has changes nothing
                net2 = copy.deepcopy(net)
                net2.zero_grad()
                out2, _ = tc.predict_train(net2, x, cfg["modes"], cfg["stages"], forced=[p.detach() for p in sums])
                F.mse_loss(out2, lb).backward()
                for (n, p), (_, q) in zip(net.named_parameters(), net2.named_parameters()):
                    assert torch.equal(p.grad, q.grad), n
                    d = tc.meets(p.grad, torch.from_numpy(fx["%s/grad64/%s" % (key, n)]), "%s %s %s" % (key, n, str(dtype)[6:]),
                                 c=tc.C / 8 if dtype == torch.float32 else 1e-12)
                    if dtype == torch.float32:
                        worst = max(worst, d)
    print("fixture batches: largest float32 distance %.3g" % worst)


def test_the_bar_is_eight_times_the_float32_torch_distance():
    """The float32 torch path against float64 over the committed op-level cases, kinks taken out: the constant the GPU tests use is 8 x
    what is measured here, and no case drops more than 10 % of its pixels."""
    worst_p, worst_x, most = 0.0, 0.0, 0.0
    for cfg in tc.OP_MODELS:
        for shape in tc.OP_SHAPES:
            for s in range(1, cfg["stages"] + 1):
                case = tc.op_case(cfg, shape, s)
                assert case["dropped"] <= tc.MAX_DROP, (tc.model_id(cfg), shape, s, case["dropped"])
                most = max(most, case["dropped"])
                gx, gp = tc.op_reference(case["net"], case["x"], case["g"], cfg["modes"], s)
                worst_x = max(worst_x, tc.distance(gx, case["gx64"]))
                worst_p = max([worst_p] + [tc.distance(gp[n], case["gp64"][n]) for n in gp])
    print("float32 torch against float64: parameters %.3g, gx %.3g of max |ref|; at most %.3g of a case's pixels dropped" % (worst_p, worst_x, most))
    assert max(worst_p, worst_x) <= tc.C / 8
    assert worst_p <= tc.MEASURED_P and worst_x <= tc.MEASURED_X


def test_kink_removal_zeroes_whole_blocks():
    g = torch.ones((1, 1, 4, 6))
    mp = torch.tensor([[[[1.0, 1e-6, 1.0], [1.0, 1.0, 0.0]]]])
    out, share = tc.kink_free(g, mp, 2)
    assert share == 2 / 6 and out.sum() == 24 - 8 and out[0, 0, 0, 2] == 0 and out[0, 0, 3, 5] == 0 and out[0, 0, 0, 0] == 1


def _unit_arrays(nf, u, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.standard_normal((nf if l < 5 else u * u, 4 if l == 0 else l * nf)).astype(np.float32) for l in range(6)]
    bs = [rng.standard_normal(nf if l < 5 else u * u).astype(np.float32) for l in range(6)]
    return ws, bs


@pytest.mark.parametrize("nf,u", [(8, 2), (33, 3), (64, 4)])
def test_backward_stream_holds_the_transposed_matrices(nf, u):
    """Through the library (mulut_net_pack_host): every step of the backward stream is a column block of a transposed weight matrix,
    placed as mulut_net.h says; everything else is zero."""
    from mulut_amd import _native
    lib = _native.load()
    fp = ctypes.POINTER(ctypes.c_float)
    ws, bs = _unit_arrays(nf, u, nf + u)
    wp, bp = (fp * 6)(*[w.ctypes.data_as(fp) for w in ws]), (fp * 6)(*[b.ctypes.data_as(fp) for b in bs])
    out = np.full(1 << 17, np.nan, np.float32)
    n = lib.mulut_net_pack_host(nf, u, wp, bp, 1, out.ctypes.data, out.size)
    MT = 1 if nf <= 32 else 2
    assert n == {1: 4, 2: 12}[MT] * 4096
    st = out[:n].reshape(-1, 64, 4).transpose(0, 2, 1).reshape(-1, 64)      # [step][lane]
    row = lambda reg, h: (reg & 3) + 8 * (reg >> 2) + 4 * h      # noqa: E731
    want = np.zeros_like(st)
    g = 0
    for s in range(5, 0, -1):
        for t in range(MT):
            feats = np.arange(32) + 32 * t
            ok = feats < nf
            cols = (s - 1) * nf + feats[ok]
            for reg in range(8):
                for h in range(2):
                    if 8 * h + reg < u * u:
                        want[g + reg, 32 * h:32 * h + 32][ok] = ws[5][8 * h + reg, cols]
            g += 8
            for L in range(5, s, -1):
                for mt in range(MT):
                    for reg in range(16):
                        for h in range(2):
                            o = 32 * mt + row(reg, h)
                            if o < nf:
                                want[g + reg, 32 * h:32 * h + 32][ok] = ws[L - 1][o, cols]
                    g += 16
    for mt in range(MT):
        for reg in range(16):
            for h in range(2):
                o = 32 * mt + row(reg, h)
                if o < nf:
                    want[g + reg, 32 * h:32 * h + 4] = ws[0][o, :4]
        g += 16
    assert g == {1: 216, 2: 752}[MT]
    assert np.array_equal(st, want)
    fwd = np.full(1 << 17, np.nan, np.float32)
    assert lib.mulut_net_pack_host(nf, u, wp, bp, 0, fwd.ctypes.data, fwd.size) == {1: 4, 2: 13}[MT] * 4096
    assert lib.mulut_net_pack_host(nf, u, wp, bp, 0, fwd.ctypes.data, 100) == -9


def test_host_half_as_a_program_under_sanitizers(tmp_path):
    """mulut_net.hip's and mulut_net_train.hip's host halves + fake_hip.cpp + net_train_host.cpp (its own main),
    -fsanitize=address,undefined, run as a program."""
    from mulut_amd import _native
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import host_abi as tool
    if _native._hipcc() is None:
        pytest.skip("no hipcc")
    assert "mulut_net_train.hip" in _native.SOURCES and "mulut_net_dev.h" in _native.HEADERS
    r = tool.run(tool.build(str(tmp_path), tool.CSRC, "net_train_host", ["mulut_net.hip", "mulut_net_train.hip"]))
    print(r.stdout)
    assert r.stderr == "", r.stderr[-4000:]
    assert r.returncode == 0 and "UNEXPECTED" not in r.stdout and r.stdout.endswith("\n0 unexpected\n")
    lines = r.stdout.splitlines()
    assert sum(ln.startswith("pack nf ") and ln.endswith(" ok") for ln in lines) == 24
    refused = [ln for ln in lines if re.search(r" -> -\d+ \[\]$", ln)]
    assert len(refused) >= 70 and {int(re.search(r"-> (-\d+) ", ln).group(1)) for ln in refused} == {-1, -4, -5, -7, -9}


def test_command_line_is_the_reference_one(tmp_path):
    from mulut_amd.options import TrainOptions
    opt = TrainOptions().parse(["-e", str(tmp_path / "e")])
    want = dict(model="SRNets", scale=4, nf=64, stages=2, modes="sdy", interval=4, batchSize=32, cropSize=48, trainDir="../data/DIV2K",
                valDir="../data/SRBenchmark", startIter=0, totalIter=200000, displayStep=100, valStep=2000, saveStep=2000, lr0=1e-3, lr1=1e-4,
                weightDecay=0, gpuNum=1, workerNum=8, torchPath=False, hostData=False, seed=None)
    assert {k: getattr(opt, k) for k in want} == want
    assert opt.valoutDir == os.path.join(str(tmp_path / "e"), "val") and os.path.isdir(opt.valoutDir) and opt.isTrain
    assert os.path.exists(os.path.join(str(tmp_path / "e"), "opt.txt"))
    dbg = TrainOptions().parse(["-e", str(tmp_path / "d"), "--debug", "--torchPath"])
    assert (dbg.displayStep, dbg.saveStep, dbg.valStep, dbg.totalIter, dbg.torchPath) == (10, 100, 50, 200, True)
    assert os.path.exists(os.path.join(ROOT, "sr", "1_train_model.py"))


def test_trainer_raises_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mulut_amd import MuLUTError
    from mulut_amd.net_train import NetTrainer
    with pytest.raises(MuLUTError):
        NetTrainer(nc.model("tiny"))


def test_header_declares_the_training_exports():
    from mulut_amd import _native
    txt = open(os.path.join(ROOT, "include", "mulut.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mulut_[a-z0-9_]+)\s*\(", txt))
    new = {"mulut_net_unit_create_train", "mulut_net_unit_load_dev", "mulut_net_unit_read", "mulut_net_pack_host", "mulut_net_stage_sum",
           "mulut_net_backward_ws_bytes", "mulut_net_stage_backward"}
    assert new <= declared and new <= set(_native.EXPORTS)
    lib = _native.load()
    assert all(hasattr(lib, n) for n in new)
    assert lib.mulut_net_backward_ws_bytes(64, 4, 128) == 16 * 46672 * 4 + 128 * 660 * 4
