"""The resident validation of the fine-tune driver without a GPU: the host halves of mulut_eval_plan_* and mulut_ft_val_pack under
sanitizers (a stand-alone program), mulut_eval_finish against mulut_amd/metrics.py, the PNG writer behind the loop, the parser."""
import ctypes
import os
import sys
import threading
import time

import numpy as np
import pytest
from PIL import Image

import val_cases as V
from conftest import ROOT
from eval_pairs import big_pairs

sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_host_half_refusals_and_launch_configuration_under_sanitizers(tmp_path):
    """mulut_eval.hip's and mulut_ft_data.hip's host halves + fake_hip.cpp + eval_list_host.cpp (its own main),
    -fsanitize=address,undefined, run as a program: every refusal in its order with *plan NULL behind it, the launch configurations of a
    1-item, a 2-item and a 328-item plan, no leak after create / destroy."""
    from mulut_amd import _native
    import host_abi as tool
    if _native._hipcc() is None:
        pytest.skip("no hipcc")
    new = {"mulut_eval_plan_create", "mulut_eval_plan_run", "mulut_eval_plan_destroy", "mulut_eval_finish", "mulut_ft_val_pack"}
    assert {"mulut_eval.hip", "mulut_ft_data.hip"} <= set(_native.SOURCES) and new <= set(_native.EXPORTS)
    r = tool.run(tool.build(str(tmp_path), tool.CSRC, "eval_list_host", ["mulut_eval.hip", "mulut_ft_data.hip"]))
    print(r.stdout)
    assert r.stderr == "", r.stderr[-4000:]
    assert r.returncode == 0 and "UNEXPECTED" not in r.stdout and r.stdout.endswith("\n0 unexpected\n")
    lines = r.stdout.splitlines()
    assert "create 1 item -> 0 [malloc 72 | memcpy 56]" in lines and "destroy 1 item -> 0 [free 72]" in lines
    assert ("run 328 items -> 0 [launch sse_list_kernel grid 328,1,1 block 256,1,1 lds 0 | launch ssim_list_kernel grid 328,1,1 block 256,1,1 lds 0 | "
            "launch eval_sum_kernel grid 328,1,1 block 64,1,1 lds 0]") in lines
    assert ("run 2 items -> 0 [launch sse_list_kernel grid 1029,1,1 block 256,1,1 lds 0 | launch ssim_list_kernel grid 260,1,1 block 256,1,1 lds 0 | "
            "launch eval_sum_kernel grid 2,1,1 block 64,1,1 lds 0]") in lines
    # the refusals of mulut_eval_plan_create in their order: arguments, shapes, pools, workgroups, device
    create = [ln for ln in lines[:lines.index("create 1 item -> 0 [malloc 72 | memcpy 56]")]]
    codes = [int(ln.split(" -> ")[1].split(" ")[0]) for ln in create]
    assert codes.count(-1) == 15 and codes.count(-4) == 7 and codes.count(-5) == 1 and codes.count(-7) == 1 and len(codes) == 24
    assert "offset -1 then H 10 -> -4 []" in lines and "too many workgroups and an offset outside -> -1 []" in lines


@pytest.fixture(scope="module")
def lib():
    from mulut_amd import _native
    return _native.load()


def _finish(lib, sse, ssim_sum, H, W, shave):
    ps, ss = ctypes.c_double(), ctypes.c_double()
    assert lib.mulut_eval_finish(sse, ssim_sum, H, W, shave, ctypes.byref(ps), ctypes.byref(ss)) == 0
    return ps.value, ss.value


def test_eval_finish_of_numpy_sums_matches_metrics(lib):
    """mulut_eval_finish (host only) of the two sums computed in NumPy against mulut_amd/metrics.py on the pairs of eval_pairs.py and
    the identical pair, within the bars of test_metrics_cpu.py: 1e-5 dB and 1e-12."""
    from mulut_amd.metrics import psnr, rgb2ycbcr, ssim
    pairs = dict(big_pairs())
    gt = pairs["tiles_minus_1"][0]
    pairs["identical"] = (gt, gt.copy(), 4)
    for name, (gt, out, shave) in pairs.items():
        sse, ssim_sum = V.numpy_sums(gt, out, shave)
        p, s = _finish(lib, sse, ssim_sum, gt.shape[0], gt.shape[1], shave)
        y_gt, y_out = rgb2ycbcr(gt)[:, :, 0], rgb2ycbcr(out)[:, :, 0]
        with np.errstate(divide="ignore"):
            want_p, want_s = float(psnr(y_gt, y_out, shave)), ssim(y_gt, y_out)
        print(name, "PSNR %.9f against %.9f, SSIM %.15f against %.15f" % (p, want_p, s, want_s))
        if name == "identical":
            assert sse == 0.0 and p == want_p == float("inf") and s == pytest.approx(1.0, abs=1e-12)
        else:
            assert p == pytest.approx(want_p, abs=1e-5), name
        assert s == pytest.approx(want_s, abs=1e-12), name


def test_eval_finish_refuses_what_eval_y_refuses(lib):
    ps, ss = ctypes.c_double(), ctypes.c_double()
    assert lib.mulut_eval_finish(1.0, 1.0, 16, 16, 4, None, ctypes.byref(ss)) == -1
    assert lib.mulut_eval_finish(1.0, 1.0, 16, 16, -1, ctypes.byref(ps), ctypes.byref(ss)) == -1
    assert lib.mulut_eval_finish(1.0, 1.0, 10, 16, 4, ctypes.byref(ps), ctypes.byref(ss)) == -4
    assert lib.mulut_eval_finish(1.0, 1.0, 16, 16, 8, ctypes.byref(ps), ctypes.byref(ss)) == -4


# --------------------------------------------------------------------------------------------------------------------- the writer
class SlowEncoder(object):
    """An injected encoder: records when each file begins and ends, holds every file until `gate` is set, fails on request."""

    def __init__(self, fail=None):
        self.gate, self.lock, self.log, self.fail = threading.Event(), threading.Lock(), [], fail

    def __call__(self, path, arr):
        with self.lock:
            self.log.append(("begin", path))
        assert self.gate.wait(30)
        if self.fail and os.path.basename(path) == self.fail:
            raise OSError("disk full: " + path)
        Image.fromarray(arr).save(path)
        with self.lock:
            self.log.append(("end", path))


def _jobs(folder, point, n=6):
    return [(os.path.join(str(folder), "%d_lutft.png" % k), np.full((5, 7, 3), 10 * point + k, np.uint8)) for k in range(n)]


def test_writer_does_not_wait_for_its_own_files_and_keeps_points_apart(tmp_path):
    from mulut_amd.finetune_lut import ValWriter
    enc = SlowEncoder()
    w = ValWriter(workers=3, encode=enc)
    t0 = time.time()
    w.submit(_jobs(tmp_path, 1))                    # returns while the encoder holds every file
    assert time.time() - t0 < 5 and not any(k == "end" for k, _ in enc.log) and os.listdir(str(tmp_path)) == []
    second = threading.Thread(target=w.submit, args=(_jobs(tmp_path, 2),))
    second.start()                                  # point 2 joins point 1 first: it cannot begin a file while point 1 is held
    second.join(0.2)
    assert second.is_alive() and sum(k == "begin" for k, _ in enc.log) <= 3
    enc.gate.set()
    second.join(30)
    assert not second.is_alive()
    w.close()
    kinds = [k for k, _ in enc.log]
    assert len(kinds) == 24
    # every file of point 1 ended before any file of point 2 began
    assert kinds[:12].count("begin") == 6 and kinds[:12].count("end") == 6 and kinds[12] == "begin"
    assert sorted(os.listdir(str(tmp_path))) == sorted("%d_lutft.png" % k for k in range(6))
    for k in range(6):                              # everything is on disk after the final join, overwritten by the later point
        assert np.array_equal(np.array(Image.open(os.path.join(str(tmp_path), "%d_lutft.png" % k))), np.full((5, 7, 3), 20 + k, np.uint8))


def test_writer_waits_for_the_copy_before_the_first_file(tmp_path):
    from mulut_amd.finetune_lut import ValWriter
    order, copied = [], threading.Event()

    def ready():
        assert copied.wait(30)
        order.append("copied")
    w = ValWriter(workers=4, encode=lambda path, arr: order.append(path))
    w.submit(_jobs(tmp_path, 1, n=5), ready=ready)
    time.sleep(0.05)
    assert order == []
    copied.set()
    w.join()
    assert order[0] == "copied" and len(order) == 6
    w.close()


def test_writer_raises_a_failed_write_at_the_next_join(tmp_path):
    from mulut_amd.finetune_lut import ValWriter
    enc = SlowEncoder(fail="2_lutft.png")
    enc.gate.set()
    w = ValWriter(workers=2, encode=enc)
    w.submit(_jobs(tmp_path, 1))
    with pytest.raises(OSError, match="disk full"):
        w.submit(_jobs(tmp_path, 2))                # the join in front of point 2
    assert sorted(os.listdir(str(tmp_path))) == ["0_lutft.png", "1_lutft.png", "3_lutft.png", "4_lutft.png", "5_lutft.png"]      # the others were written
    w.join()                                        # raised once, not again
    enc.fail = "4_lutft.png"
    w.submit(_jobs(tmp_path, 3))
    with pytest.raises(OSError, match="disk full"):
        w.close()                                   # the final join


def test_file_names_follow_the_references_last_token_rule():
    from mulut_amd.finetune_lut import val_png_name
    assert val_png_name("Urban100", "img_001.png") == "001_lutft.png"
    assert val_png_name("Set5", "baby.png") == "baby_lutft.png"                 # "Set5_baby" -> "baby"
    assert val_png_name("Set14", "ppt3.png") == "ppt3_lutft.png"
    assert val_png_name("Manga109", "Akkera_Kanjinchou.png") == "Kanjinchou_lutft.png"


# --------------------------------------------------------------------------------------------------------------------- the parser
def test_parser_defaults_and_choices(tmp_path, monkeypatch):
    from mulut_amd import finetune_lut
    base = ["-e", str(tmp_path)]
    opt = finetune_lut.build_parser().parse_args(base)
    assert opt.valResident is False and opt.valSave == "every" and opt.valWorkers == 4 and opt.valMaxBytes is None
    assert finetune_lut.build_parser().parse_args(base + ["--valResident"]).valResident is True
    for v in ("every", "last", "never"):
        assert finetune_lut.build_parser().parse_args(base + ["--valSave", v]).valSave == v
    with pytest.raises(SystemExit):
        finetune_lut.build_parser().parse_args(base + ["--valSave", "sometimes"])
    for cpus in (1, 16, 384):                       # never sized from the machine
        monkeypatch.setattr(os, "cpu_count", lambda: cpus)
        assert finetune_lut.build_parser().parse_args(base).valWorkers == 4
    assert finetune_lut.build_parser().parse_args(base + ["--valWorkers", "7"]).valWorkers == 7


def test_val_save_names_the_final_point():
    import argparse
    from mulut_amd.finetune_lut import _val_saves
    opt = argparse.Namespace(valSave="last", totalIter=4, valStep=2)
    assert [it for it in (1, 2, 4) if _val_saves(opt, it)] == [4]
    opt = argparse.Namespace(valSave="last", totalIter=5000, valStep=2000)
    assert [it for it in (1, 2000, 4000) if _val_saves(opt, it)] == [4000]
    opt = argparse.Namespace(valSave="last", totalIter=10, valStep=50)
    assert _val_saves(opt, 1)
    assert _val_saves(argparse.Namespace(valSave="every", totalIter=4, valStep=2), 1)
    assert not _val_saves(argparse.Namespace(valSave="never", totalIter=4, valStep=2), 4)
