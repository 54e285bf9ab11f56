"""The list form of the cascade and the resident validation of network training without a GPU: the host half of mulut_net_plan_* under
sanitizers (a stand-alone program), the plan's tables against a restatement, the parsers' new flags, DeviceValSet's byte count."""
import os
import subprocess
import sys

import pytest

import net_list_cases as L
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """mulut_net.hip's and mulut_net_list.hip's host halves + fake_hip.cpp + net_list_host.cpp (its own main), built with
    -fsanitize=address,undefined."""
    from mulut_amd import _native
    import host_abi as tool
    if _native._hipcc() is None:
        pytest.skip("no hipcc")
    new = {"mulut_net_plan_create", "mulut_net_plan_run", "mulut_net_plan_destroy"}
    assert "mulut_net_list.hip" in _native.SOURCES and "mulut_net_list.h" in _native.HEADERS and new <= set(_native.EXPORTS)
    return tool, tool.build(str(tmp_path_factory.mktemp("net_list_host")), tool.CSRC, "net_list_host", ["mulut_net.hip", "mulut_net_list.hip"])


def test_host_half_refusals_and_launches_under_sanitizers(program):
    """Every refusal of create with *plan NULL behind it and of run, none with an event; the order of the classes where two codes tell
    it; `stages` launches and nothing else in a run of 1, 2 and 3 stages, each over the list's workgroups; no leak."""
    tool, exe = program
    r = tool.run(exe)
    print(r.stdout)
    assert r.stderr == "", r.stderr[-4000:]
    assert r.returncode == 0 and "UNEXPECTED" not in r.stdout and r.stdout.endswith("\n0 unexpected\n")
    lines = r.stdout.splitlines()
    # create's refusals in their order: arguments, empty items, pools, overlaps, counts, device
    create = [ln for ln in lines[:lines.index("device 3 -> -7 []") + 1] if " -> " in ln and not ln.startswith("  ") and "ends with its pool" not in ln
              and not ln.startswith("results that touch")]
    codes = [int(ln.split(" -> ")[1].split(" ")[0]) for ln in create]
    assert codes.count(-1) == 26 and codes.count(-5) == 4 and codes.count(-7) == 1 and len(codes) == 31, codes
    assert all(ln.endswith(" []") for ln in create)
    assert lines.count("  plan is NULL ok") == 30      # (the call with a NULL `plan` has nowhere to write it)
    for ln in ("2^31 result bytes then h 0 -> -1 []", "2^31 result bytes then in_off -1 -> -1 []", "2^31 result bytes then an overlap -> -1 []",
               "an item of 2^31 result bytes on device 3 -> -5 []", "2^31 workgroups -> -5 []", "a workspace of 2^31 bytes -> -5 []"):
        assert ln in lines, ln
    # a run is `stages` launches and nothing else: no allocation, no copy, no wait
    launch = "launch net_list_kernel<%d, %d> grid %d,1,1 block 256,1,1 lds 0"
    assert "run 1 stage -> 0 [%s]" % (launch % (1, 4, 1)) in lines
    assert "run 2 stages -> 0 [%s | %s]" % (launch % (1, 1, 1), launch % (1, 4, 1)) in lines
    assert "run 3 stages -> 0 [%s | %s | %s]" % (launch % (2, 1, 12), launch % (1, 1, 12), launch % (2, 4, 12)) in lines
    assert "run 328 items -> 0 [%s | %s]" % (launch % (1, 1, 656), launch % (1, 4, 656)) in lines
    runs = [ln for ln in lines if ln.startswith("run ")]
    assert len(runs) == 19 and not any(w in ln for ln in runs for w in ("malloc", "memcpy", "memset", "wait", "free", "event"))
    refused = [ln for ln in runs if not ln.split(" -> ")[1].startswith("0 ")]
    assert len(refused) == 14 and all(ln.endswith(" []") for ln in refused)
    # the workspace: 32 bytes an item, 8 a workgroup, no plane set for one stage, one for two, two for more
    assert "create 1 stage -> 0 [malloc 40 | memcpy 40]" in lines and "create 2 stages -> 0 [malloc 145 | memcpy 40]" in lines
    assert "create 3 stages, 7 items -> 0 [malloc 2132 | memcpy 320]" in lines and "destroy 3 stages -> 0 [free 2132]" in lines
    assert L.tables(L.MIXED, 3, 3, 4)[2:] == (2132, 320) and L.tables([(6, 8)] * 328, 3, 2, 4)[2:] == (62976, 15744)


@pytest.mark.parametrize("name,shapes,ch,stages,scale", [("mixed", L.MIXED, 3, 2, 4), ("mixed, one stage", L.MIXED, 3, 1, 2), ("mixed, grey, 3 stages", L.MIXED, 1, 3, 3),
                                                         ("many", L.MANY, 3, 2, 4), ("one pixel", [(1, 1)], 1, 4, 1)])
def test_tables_of_a_plan_against_the_restatement(program, name, shapes, ch, stages, scale):
    """The item table and the workgroup map as the device would read them (`tables` mode of the program), the allocation and the copy,
    against net_list_cases.tables: per item its offsets, the planes' offset and the size; per workgroup (item, first site)."""
    tool, exe = program
    r = tool.run(exe, "tables", str(ch), str(stages), str(scale), *["%dx%d" % s for s in shapes])
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    items, wg_map, ws, copied = L.tables(shapes, ch, stages, scale)
    assert lines[0] == "create 0 | malloc %d | memcpy %d" % (ws, copied)
    sites = sum(ch * h * w for h, w in shapes)
    assert lines[1] == "groups %d set_bytes %d map_at %d planes_at %d" % (len(wg_map), sites, 32 * len(items), copied)
    got_items = [tuple(int(v) for v in ln.split(": ")[1].split()) for ln in lines[2:2 + len(items)]]
    assert got_items == items
    got_map = [tuple(int(v) for v in e.split(":")) for e in lines[2 + len(items)].split()[1:]]
    assert got_map == wg_map
    # the restatement restated: per-item workgroup counts, and every workgroup's sites lie inside its item
    counts = [sum(1 for i, _ in got_map if i == k) for k in range(len(shapes))]
    assert counts == [-(-ch * h * w // L.SITES) for h, w in shapes]
    assert all(s % L.SITES == 0 and s < ch * shapes[i][0] * shapes[i][1] for i, s in got_map)
    if name == "many":
        assert len(got_map) > 512


def test_train_and_transfer_parsers_take_the_resident_flags(tmp_path):
    """--valResident, --valSave every|last|never, --valWorkers: the words and defaults of the fine-tune parser, in TrainOptions and
    in transfer_to_lut's options."""
    from mulut_amd import finetune_lut
    from mulut_amd.options import TrainOptions
    from mulut_amd.transfer_to_lut import TransferOptions
    ft = finetune_lut.build_parser()
    for k, (cls, base) in enumerate(((TrainOptions, []), (TransferOptions, ["--fused"]))):
        e = ["-e", str(tmp_path / ("e%d" % k))]
        opt = cls().parse(e + base)
        assert opt.valResident is False and opt.valSave == "every" and opt.valWorkers == 4
        for flag in ("valResident", "valSave", "valWorkers"):
            assert getattr(opt, flag) == ft.get_default(flag)
        opt = cls().parse(e + base + ["--valResident", "--valSave", "last", "--valWorkers", "7"])
        assert opt.valResident is True and opt.valSave == "last" and opt.valWorkers == 7
        assert cls().parse(e + base + ["--valSave", "never"]).valSave == "never"
        with pytest.raises(SystemExit):
            cls().parse(e + base + ["--valSave", "sometimes"])
    ours = {a.dest: a for a in TrainOptions().initialize(__import__("argparse").ArgumentParser())._actions}
    theirs = {a.dest: a for a in ft._actions}
    for f in ("valResident", "valSave", "valWorkers"):      # the flags, not the help: the network's point scores on the host, and says so
        assert (ours[f].option_strings, ours[f].default, ours[f].choices, ours[f].type) == (theirs[f].option_strings, theirs[f].default, theirs[f].choices, theirs[f].type)
    assert "scored on the host" in ours["valResident"].help and "score" in ours["valWorkers"].help


def test_device_val_set_byte_count_with_and_without_the_float_pool():
    """Arithmetic only: ground truths and results, the LR bytes, and 4 more bytes per LR byte for the float32 pool."""
    from mulut_amd.ft_val import DeviceValSet
    gt, lr = 16 * 3 * 1000, 3 * 1000
    assert DeviceValSet.pool_bytes(gt, lr) == DeviceValSet.pool_bytes(gt, lr, True) == 2 * gt + 5 * lr
    assert DeviceValSet.pool_bytes(gt, lr, False) == 2 * gt + lr
    assert DeviceValSet.pool_bytes(gt, lr) - DeviceValSet.pool_bytes(gt, lr, False) == 4 * lr
    import inspect
    sig = inspect.signature(DeviceValSet.__init__)
    assert sig.parameters["lr_float"].default is True and sig.parameters["png_name"].default is None and sig.parameters["eval_plans"].default is True


def test_net_png_names():
    """The last '_'-separated token of "{dataset}_{stem}" with the training script's three suffixes."""
    from mulut_amd.net_val import net_png_name
    assert net_png_name("Urban100", "img_001.png") == "001_net.png" and net_png_name("Set5", "baby.png", "gt") == "baby_gt.png"
    assert net_png_name("Set14", "zz_odd.png", "input") == "odd_input.png"


def test_luma32_is_the_y_plane_metrics_psnr_takes():
    """net_val.luma32 against np.array(rgb2ycbcr(img)[:, :, 0], dtype=np.float32), bit for bit, on every byte triple of a random image
    and on the corners of the cube; psnr of the two forms is the same numpy.float32."""
    import numpy as np
    from mulut_amd.metrics import psnr, rgb2ycbcr
    from mulut_amd.net_val import luma32
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, (61, 47, 3), dtype=np.uint8), rng.integers(0, 256, (61, 47, 3), dtype=np.uint8)
    a[0, :8] = [[r, g, c] for r in (0, 255) for g in (0, 255) for c in (0, 255)]
    for img in (a, b):
        want = np.array(rgb2ycbcr(img)[:, :, 0], dtype=np.float32)
        got = luma32(img)
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    x, y = psnr(rgb2ycbcr(a)[:, :, 0], rgb2ycbcr(b)[:, :, 0], 4), psnr(luma32(a), luma32(b), 4)
    assert type(x) is type(y) and x == y
