"""The fused network forward without a GPU: what tests/golden/net_fixtures.npz (gen_golden_net.py: the reference's own mulut_predict /
round_func over its SRNets) holds, the torch restatement of tests/net_cases.py against it, the host half of mulut_net_* as a program
of its own under sanitizers, the command line, and the refusal to run without a GPU.

The bar is net_cases.py's.  It is a share of values, so it is taken over all the values of a kind that a model has in the fixture
(every per-pass value of every case and stage; every stage byte; every result byte) -- at least 100,000 bytes per model, so a cap is
tens to hundreds of values; on one 1 x 9 array a single legitimate flip would be a share of 1 / 36."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import net_cases as nc


def test_the_fixture_holds_what_it_claims():
    fx = nc.fixture()
    want_shapes = {"1x1": (1, 1), "1x9": (1, 9), "9x1": (9, 1), "5x7": (5, 7), "33x65": (33, 65), "65x33": (65, 33)}
    for name, cfg in nc.MODELS.items():
        cases, M, total = nc.cases(name), len(cfg["modes"]), 0
        assert set(want_shapes) <= set(cases)
        xs = [fx["%s/%s/x" % (name, c)] for c in cases]
        assert {x.shape[1] for x in xs} == {1, 3} and max(x.shape[0] for x in xs) == 2 and all(x.dtype == np.uint8 for x in xs)
        for c, x in zip(cases, xs):
            if c in want_shapes:
                assert x.shape[2:] == want_shapes[c]
            N, C, H, W = x.shape
            for s in range(1, cfg["stages"] + 1):
                u = cfg["scale"] if s == cfg["stages"] else 1
                p, out = fx["%s/%s/s%d/pass" % (name, c, s)], fx["%s/%s/s%d/out" % (name, c, s)]
                assert p.dtype == np.int8 and p.shape == (4 * M, N, C, H * u, W * u) and out.dtype == np.uint8 and out.shape == p.shape[1:]
                assert p.min() >= -127
                # the per-pass arrays sum to the stage's bytes through the integer epilogue: exactly
                assert np.array_equal(nc.epilogue(p, s == cfg["stages"]), out), (name, c, s)
                total += out.size
            differs, of = fx["%s/%s/f64_share" % (name, c)]
            assert of == fx["%s/%s/s%d/out" % (name, c, cfg["stages"])].size and differs <= max(1, 1e-4 * of)
        assert total >= 100000, (name, total)
    assert abs(np.mean([fx["set5/%s/psnr" % n] for n in nc.SET5]) - fx["set5/train_log_psnr"]) < 5e-3
    assert float(fx["set5/train_log_psnr"]) == 30.607945948346618
    for path in os.listdir(os.path.join(ROOT, "tests", "golden")):
        if path.startswith("net_fixtures"):
            assert os.path.getsize(os.path.join(ROOT, "tests", "golden", path)) < (1 << 20)


def test_integer_epilogue_is_the_float32_one():
    """Every pred a stage of up to 8 modes can produce, through the reference's float32 expressions and through the integer
    round-half-even of the rational: the same byte."""
    for M in range(1, 9):
        pred = torch.arange(-127 * 4 * M, 127 * 4 * M + 1, dtype=torch.float32)
        passes = np.zeros((4 * M, pred.numel()), np.int64)      # (one pass value per element stands for the sum: epilogue() only sums)
        passes[0] = pred.numpy().astype(np.int64)
        mid = torch.round(torch.clamp(pred / (4 * M) + 127, 0, 255)).numpy().astype(np.uint8)
        last = np.round(np.clip(torch.round(pred / M).numpy(), 0, 255)).astype(np.uint8)
        assert np.array_equal(nc.epilogue(passes, False), mid) and np.array_equal(nc.epilogue(passes, True), last), M


def test_restatement_meets_the_bar_on_the_cpu():
    fx = nc.fixture()
    for name, cfg in nc.MODELS.items():
        net, S = nc.model(name), cfg["stages"]
        got_p, want_p, got_stage, want_stage, got_end, want_end = [], [], [], [], [], []
        for c in nc.cases(name):
            x = torch.from_numpy(fx["%s/%s/x" % (name, c)])
            for s, (p, out) in enumerate(nc.predict_valid(net, x, cfg["modes"], S), 1):      # the cascade on its own bytes
                if s == S:
                    got_end.append(out.numpy().ravel())
                    want_end.append(fx["%s/%s/s%d/out" % (name, c, s)].ravel())
            for s in range(1, S + 1):                                                        # each stage on the reference's input bytes
                xin = x if s == 1 else torch.from_numpy(fx["%s/%s/s%d/out" % (name, c, s - 1)])
                p, out = _one_stage(net, xin, cfg["modes"], s, S)
                got_p.append(p.numpy().ravel())
                want_p.append(fx["%s/%s/s%d/pass" % (name, c, s)].ravel())
                got_stage.append(out.numpy().ravel())
                want_stage.append(fx["%s/%s/s%d/out" % (name, c, s)].ravel())
        M = len(cfg["modes"])
        nc.meets(np.concatenate(got_p), np.concatenate(want_p), nc.BAR, name + " passes")
        nc.meets(np.concatenate(got_stage), np.concatenate(want_stage), 4 * M * nc.BAR, name + " stages")
        nc.meets(np.concatenate(got_end), np.concatenate(want_end), S * 4 * M * nc.BAR, name + " cascade", by_one=False)


def _one_stage(net, x_u8, modes, s, stages):
    """Stage s alone: predict_valid of a one-stage view of the model."""
    class View:
        def __call__(self, x, stage, mode):
            return net(x, stage=s, mode=mode)
    p, out = nc.predict_valid(View(), x_u8, modes, 1)[0]
    if s != stages:      # a one-stage view ends in the final epilogue: redo the non-final one from the passes
        out = torch.from_numpy(nc.epilogue(p.numpy(), False))
    return p, out


def test_host_half_as_a_program_under_sanitizers(tmp_path):
    """mulut_net.hip's host half + fake_hip.cpp + net_host.cpp (its own main), -fsanitize=address,undefined, run as a program: the pack
    walked as the kernel walks it against a plain-loop MLP, the zero padding, every refusal, allocations and launch configurations."""
    from mulut_amd import _native
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import host_abi as tool
    if _native._hipcc() is None:
        pytest.skip("no hipcc")
    assert "mulut_net.hip" in _native.SOURCES and "mulut_net.h" in _native.HEADERS
    r = tool.run(tool.build(str(tmp_path), tool.CSRC, "net_host", ["mulut_net.hip"]))
    print(r.stdout)
    assert r.stderr == "", r.stderr[-4000:]
    assert r.returncode == 0 and "UNEXPECTED" not in r.stdout and r.stdout.endswith("\n0 unexpected\n")
    lines = r.stdout.splitlines()
    assert sum(ln.startswith("pack nf ") and ln.endswith(" ok") for ln in lines) == 24
    assert any(ln.startswith("pack nf 8 u 2: 248 steps in 4 chunks") for ln in lines)
    assert "create nf 64 u 4 -> 0 [malloc 212992 | memcpy 212992]" in lines and "destroy nf 8 -> 0 [free 65536]" in lines
    assert "table interval 4 -> 0 [launch net_table_kernel<2, 4> grid 653,1,1 block 256,1,1 lds 0]" in lines
    assert "table interval 5 -> 0 [launch net_table_kernel<2, 4> grid 52,1,1 block 256,1,1 lds 0]" in lines
    assert "table interval 6 -> 0 [launch net_table_kernel<1, 2> grid 5,1,1 block 256,1,1 lds 0]" in lines
    assert "stage sd 65 x 33 x 3 x 2 -> 0 [launch net_stage_kernel<2, 4> grid 101,1,1 block 256,1,1 lds 0]" in lines
    refused = [ln for ln in lines if re.search(r" -> -\d+ \[\]$", ln)]
    assert len(refused) >= 60 and {int(re.search(r"-> (-\d+) ", ln).group(1)) for ln in refused} == {-1, -4, -5, -7}


def test_command_line_parses_the_new_flags(tmp_path):
    from mulut_amd import transfer_to_lut as T
    opt = T.TransferOptions().parse(["-e", str(tmp_path), "--fused", "--valDir", "bench", "--valoutDir", "out"])
    assert opt.fused is True and opt.valDir == "bench" and opt.valoutDir == "out"
    opt = T.TransferOptions().parse(["-e", str(tmp_path)])
    assert opt.fused is False and opt.valDir is None and opt.valoutDir is None and opt.interval == 4      # nothing changes without the flag
    from mulut_amd.net_val import net_png_name
    assert net_png_name("Set5", "baby.png") == "baby_net.png" and net_png_name("Urban100", "img_001.png", "gt") == "001_gt.png"


def test_transfer_takes_tables_from_a_net_engine(tmp_path):
    """transfer(net_engine=) asks the engine for every table and keeps names and shapes; here the engine is a stand-in."""
    from types import SimpleNamespace
    from mulut_amd import transfer_to_lut as T
    asked = []

    class Stand:
        def table(self, stage, mode, interval):
            asked.append((stage, mode, interval))
            u = 2 if stage == 2 else 1
            return torch.full((83521, 1, u, u), stage, dtype=torch.int8)
    opt = SimpleNamespace(stages=2, modes="sd", scale=2, interval=4, expDir=str(tmp_path))
    tabs = T.transfer(None, opt, net_engine=Stand())
    assert asked == [(1, "s", 4), (1, "d", 4), (2, "s", 4), (2, "d", 4)]
    assert tabs["s2_d"].shape == (83521, 1, 2, 2) and tabs["s2_d"].dtype == np.int8
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "LUT_x2_4bit_int8_s2_d.npy")), tabs["s2_d"])


def test_net_engine_raises_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mulut_amd import MuLUTError
    from mulut_amd.net_engine import NetEngine
    with pytest.raises(MuLUTError):
        NetEngine(nc.model("tiny"))


def test_header_declares_exactly_the_exports():
    from mulut_amd import _native
    txt = open(os.path.join(ROOT, "include", "mulut.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mulut_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(_native.EXPORTS) == declared
    new = {"mulut_net_unit_create", "mulut_net_unit_destroy", "mulut_net_table", "mulut_net_pass", "mulut_net_stage"}
    assert new <= set(declared)
    lib = _native.load()
    assert all(hasattr(lib, n) for n in new)
