"""The bit-reproducible backward of the SR network without a GPU: the host model of the gather-form input gradient
(tests/host_emul/net_gx_host.cpp) against torch autograd, exactly; the header and the library's three new exports; the host halves of
those entry points as a program of its own under sanitizers; the command line."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

from mulut_amd import network
import net_cases as nc
import net_exact_cases as xc


@pytest.mark.parametrize("mode", xc.LETTERS)
def test_host_model_is_the_reference_expression(mode):
    """Integer-valued t below 2^10: every float32 sum of a pixel's at most 64 terms is exact in any order, so the model's gx must
    EQUAL autograd's gradient of sum_k t_k * tap_k(pad(rot90^r(x))), the taps cut as net_train_cases.stage_terms cuts them
    (sr/1_train_model.py:33-35).  This pins the model's index arithmetic with no GPU."""
    pad, offs = network.TAPS[mode.upper()][0] - 1, network.TAPS[mode.upper()][1]
    rng = np.random.default_rng(ord(mode))
    for shape in xc.OP_SHAPES:
        N, C, H, W = shape
        total = N * C * H * W
        for r in range(4):
            for ts in (total, total + 128):
                t = np.zeros((4, ts), np.float32)
                t[:, :total] = rng.integers(-1023, 1024, (4, total))
                t[:, total:] = np.nan      # rows beyond the last site are never read
                x = torch.zeros(shape, requires_grad=True)
                xp = F.pad(torch.rot90(x, r, [2, 3]), (0, pad, 0, pad), mode="replicate")
                h, w = xp.shape[2] - pad, xp.shape[3] - pad
                loss = 0
                for k, (i, j) in enumerate(offs):
                    tk = torch.rot90(torch.from_numpy(t[k, :total].reshape(shape)), r, [2, 3])      # the site of a pixel: its place in the rotated frame
                    loss = loss + (tk * xp[:, :, i:i + h, j:j + w]).sum()
                loss.backward()
                got = xc.host_pass(mode, r, t, shape)
                assert np.array_equal(got, x.grad.numpy()), (mode, r, shape, ts)
                # added to what is there, and a stage is its passes chained
                base = rng.integers(-1023, 1024, shape).astype(np.float32)
                assert np.array_equal(xc.host_pass(mode, r, t, shape, gx=base), base + got)
    shape = (2, 3, 5, 7)
    t = rng.integers(-1023, 1024, (8, 4, 210 + 128)).astype(np.float32)
    want = sum(xc.host_pass(m, r, t[4 * mi + r], shape) for mi, m in enumerate(mode + "s") for r in range(4))
    assert np.array_equal(xc.host_stage(mode + "s", t, shape), want)


def test_header_declares_the_exact_exports():
    from mulut_amd import _native
    txt = open(os.path.join(ROOT, "include", "mulut.h")).read()
    assert "acc = acc + t[k][plane * H * W + s]" in txt and "acc = accumulate ? gx[p] : +0.0f" in txt      # the contract, word for word
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mulut_[a-z0-9_]+)\s*\(", txt))
    new = {"mulut_net_backward_exact_ws_bytes", "mulut_net_stage_backward_exact", "mulut_net_gx_gather"}
    assert new <= declared and new <= set(_native.EXPORTS)
    lib = _native.load()
    assert all(hasattr(lib, n) for n in new)
    # the old figure plus 16 bytes per site of the whole pass, sites rounded up to 128
    old = lib.mulut_net_backward_ws_bytes
    assert old(64, 4, 128) == 16 * 46672 * 4 + 128 * 660 * 4      # (what tests/test_net_train_cpu.py pins)
    assert lib.mulut_net_backward_exact_ws_bytes(64, 4, 128, 128) == old(64, 4, 128) + 16 * 128
    assert lib.mulut_net_backward_exact_ws_bytes(64, 4, 128, 200) == old(64, 4, 128) + 16 * 256
    assert lib.mulut_net_backward_exact_ws_bytes(64, 4, 65536, 73728) == old(64, 4, 65536) + 16 * 73728
    assert lib.mulut_net_backward_exact_ws_bytes(24, 2, 1000, 1001) == old(24, 2, 1000) + 16 * 1024
    assert lib.mulut_net_backward_exact_ws_bytes(64, 4, 128, 0) == -1 and lib.mulut_net_backward_exact_ws_bytes(64, 4, 0, 128) == -1
    assert lib.mulut_net_backward_exact_ws_bytes(65, 4, 128, 128) == -5 and lib.mulut_net_backward_exact_ws_bytes(64, 4, 128, 1 << 31) == -5


def test_host_half_as_a_program_under_sanitizers(tmp_path):
    """mulut_net.hip's and mulut_net_train.hip's host halves + fake_hip.cpp + net_gx_host.cpp (its own main),
    -fsanitize=address,undefined, run as a program: the model's scatter against the contract's gather by search, every refusal of the
    three new calls without a launch, the launch sequences of the exact backward."""
    from mulut_amd import _native
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import host_abi as tool
    if _native._hipcc() is None:
        pytest.skip("no hipcc")
    r = tool.run(tool.build(str(tmp_path), tool.CSRC, "net_gx_host", ["mulut_net.hip", "mulut_net_train.hip"], flags=["-ffp-contract=off"]))
    print(r.stdout)
    assert r.stderr == "", r.stderr[-4000:]
    assert r.returncode == 0 and "UNEXPECTED" not in r.stdout and r.stdout.endswith("\n0 unexpected\n")
    lines = r.stdout.splitlines()
    assert sum(ln.startswith("model ") and ln.endswith(" ok") for ln in lines) == 13
    refused = [ln for ln in lines if re.search(r" -> -\d+ \[\]$", ln)]
    assert len(refused) >= 45 and {int(re.search(r"-> (-\d+) ", ln).group(1)) for ln in refused} == {-1, -4, -5, -7, -9}
    ran = [ln for ln in lines if ln.startswith("exact ") and "launch" in ln]
    assert len(ran) == 4 and all("net_bwd_site_taps_kernel" in ln and "net_bwd_site_kernel" not in ln for ln in ran)
    assert [ln.count("net_gx_gather_kernel") for ln in ran] == [4, 0, 8, 4]


def test_command_line_has_the_two_flags(tmp_path):
    from mulut_amd import train_model
    from mulut_amd.options import TrainOptions
    opt = TrainOptions().parse(["-e", str(tmp_path / "e")])
    assert opt.deterministic is False and opt.saveOpt is False
    opt = TrainOptions().parse(["-e", str(tmp_path / "f"), "--deterministic", "--saveOpt"])
    assert opt.deterministic is True and opt.saveOpt is True and opt.torchPath is False and opt.seed is None
    both = TrainOptions().parse(["-e", str(tmp_path / "g"), "--deterministic", "--torchPath"])
    with pytest.raises(SystemExit, match="--deterministic .* --torchPath"):
        train_model.train(both, lambda s: None)
    two = TrainOptions().parse(["-e", str(tmp_path / "h"), "--deterministic", "--gpuNum", "2"])
    with pytest.raises(SystemExit, match="one GPU"):
        train_model.train(two, lambda s: None)


def test_deterministic_trainer_raises_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mulut_amd import MuLUTError
    from mulut_amd.net_train import NetTrainer
    with pytest.raises(MuLUTError):
        NetTrainer(nc.model("tiny"), deterministic=True)
