"""Sampling intervals 5 and 6 on the GPU (-m gpu): every stage of a context configured at those intervals runs on
stage_interval_kernel (mulut_interval.hip), passes on pass_kernel<IV> (mulut_kernels.hip).  Checked bit-exactly against the C oracle (generic in the
interval) for s, d, y lists and against the host emulator of mulut_interval.h (tests/host_emul/emul_interval.cpp) for lists with
e, h, o."""
import os

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN
from oracle import c_oracle, np_port
from test_interval_cpu import emul_iv, fixture_luts, fixture_passes, ivfx, run_emul_iv, sha256_i32  # noqa: F401  (emulator, fixtures)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine, MuLUTError, lut_io, synthetic_lut  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def make_luts(stages, modes, scale, interval, seed=0):
    return {"s%d_%s" % (s + 1, m): synthetic_lut(seed + 31 * s + ord(m), scale * scale if s + 1 == stages else 1, interval)
            for s in range(stages) for m in modes}


def engine(stages, modes, scale, interval, luts):
    return MuLUTEngine(0).configure(stages, modes, scale, interval).set_lut_dict(luts)


def emul_pipeline(L, luts, stages, modes, scale, interval, img_hwc):
    cur = np.ascontiguousarray(img_hwc)
    for s in range(stages):
        last = s + 1 == stages
        cur = run_emul_iv(L, [luts["s%d_%s" % (s + 1, m)] for m in modes], modes, last, cur, scale if last else 1, interval)
    return cur


def natural_noise(H, W, seed):
    """Left half D-natural, right half uniform noise: both the smooth and the detailed regime in one image."""
    img = natural_frames(1, H, W, 3, seed=seed)[0]
    img[:, W // 2:] = np.random.default_rng(seed).integers(0, 256, (H, W - W // 2, 3), dtype=np.uint8)
    return img


# ---------------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------------
def test_configure_accepts_intervals_5_and_6_only():
    e = MuLUTEngine(0)
    for iv in (5, 6, 4):
        e.configure(2, "sdy", 4, iv)
    for iv in (2, 3, 7):
        with pytest.raises(MuLUTError):
            e.configure(2, "sdy", 4, iv)
    e.configure(2, "sdy", 4, 5)
    with pytest.raises(MuLUTError, match="shape"):          # an interval-4 table at interval 5
        e.set_lut(1, "s", synthetic_lut(0, 1))
    with pytest.raises(MuLUTError, match="shape"):
        e.set_lut(1, "s", synthetic_lut(0, 1, interval=6))
    e.set_lut(1, "s", synthetic_lut(0, 1, interval=5))
    e.close()


@pytest.mark.parametrize("interval", [5, 6])
@pytest.mark.parametrize("u", [1, 2, 3, 4])
def test_pass_matches_oracle_all_modes_and_rotations(interval, u):
    rng = np.random.default_rng(interval * 10 + u)
    e = MuLUTEngine(0)
    for mode in "sdy":
        e.configure(1, mode, u, interval)
        lut = rng.integers(-128, 128, (lut_io.lut_rows(interval), u * u), dtype=np.int8)
        e.set_lut(1, mode, lut)
        for shape in ((3, 19, 13), (1, 8, 31), (2, 5, 4), (1, 1, 1)):
            img = rng.integers(0, 256, shape, dtype=np.uint8)
            img.flat[:3] = (0, 255, 2 ** interval)
            for r in range(4):
                got = e.pass_q(1, mode, r, dev(img)).cpu().numpy()
                assert np.array_equal(got, c_oracle.pass_q(lut, img, r, u, mode, interval=interval)), (mode, shape, r)
    e.close()


@pytest.mark.parametrize("interval", [5, 6])
def test_interp_twin_matches_np_port(interval):
    from mulut_amd.interp import FourSimplexInterpFaster
    rng = np.random.default_rng(interval)
    for mode, u in (("s", 4), ("d", 1), ("y", 2)):
        w = rng.integers(-127, 128, (lut_io.lut_rows(interval), u * u)).astype(np.float32)
        img = rng.integers(0, 256, (3, 10, 12), dtype=np.uint8)
        for r in range(4):
            rimg = np.rot90(img, r, (1, 2))
            h, wd = rimg.shape[1:]
            p = np_port.PAD[mode]
            img_in = np.pad(rimg, ((0, 0), (0, p), (0, p)), mode="edge").astype(np.float32)
            got = FourSimplexInterpFaster(w, img_in, h, wd, interval, 4 - r, upscale=u, mode=mode)
            want = np_port.four_simplex_interp(w, img_in, h, wd, interval, 4 - r, upscale=u, mode=mode)
            assert np.array_equal(got, want), (mode, u, r)


@pytest.mark.parametrize("interval", [5, 6])
def test_pass_and_interp_twin_match_reference_fixtures(ivfx, interval):  # noqa: F811
    from mulut_amd.interp import FourSimplexInterpFaster
    luts = fixture_luts(ivfx, interval)
    e = MuLUTEngine(0)
    cases = fixture_passes(ivfx, interval)
    assert len(cases) == 6 * 2 * 3 * 4
    for name, u, mode, r, sha, arr in cases:
        img = ivfx["iv%d/in/%s" % (interval, name)]
        lut = luts["s%d_%s" % (1 if u == 1 else 2, mode)]
        e.configure(1, mode, u, interval)
        e.set_lut(1, mode, lut)
        got = e.pass_q(1, mode, r, dev(img.transpose(2, 0, 1))).cpu().numpy()
        assert sha256_i32(got) == sha, ("mulut_pass", name, u, mode, r)
        if arr is not None:
            assert np.array_equal(got, arr), ("mulut_pass", name, u, mode, r)
        # the twin, called as the reference's driver calls FourSimplexInterpFaster (sr/4_test_lut.py:289-298)
        rimg = np.rot90(img.astype(np.float32), r)
        h, w, _ = rimg.shape
        pad = np_port.PAD[mode]
        img_in = np.pad(rimg, ((0, pad), (0, pad), (0, 0)), mode="edge").transpose(2, 0, 1)
        tw = FourSimplexInterpFaster(lut.astype(np.float32), img_in, h, w, interval, 4 - r, upscale=u, mode=mode)
        assert sha256_i32(np.rint(tw * 2 ** interval)) == sha, ("interp", name, u, mode, r)
    e.close()


@pytest.mark.parametrize("interval", [5, 6])
def test_cascade_matches_reference_crop(ivfx, interval):  # noqa: F811
    import hashlib
    luts = fixture_luts(ivfx, interval)
    e = engine(2, "sdy", 4, interval, luts)
    img = dev(ivfx["in/crop"])
    assert np.array_equal(e.stage(1, img).cpu().numpy(), ivfx["iv%d/crop/stage1" % interval])
    fin = e.pipeline(img).cpu().numpy()
    assert hashlib.sha256(np.ascontiguousarray(fin).tobytes()).hexdigest() == str(ivfx["iv%d/crop/final_sha256" % interval])
    e.close()


# ---------------------------------------------------------------------------------------------
# cascades against the C oracle; both table routes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", [5, 6])
@pytest.mark.parametrize("stages,scale", [(1, 1), (1, 4), (2, 4), (2, 3), (3, 2), (4, 4)])
@pytest.mark.parametrize("modes", ["s", "sdy", "sdysdyds"])
def test_pipeline_matches_oracle(interval, stages, scale, modes):
    luts = make_luts(stages, modes, scale, interval, seed=stages + scale)
    e = engine(stages, modes, scale, interval, luts)
    rng = np.random.default_rng(stages * 7 + scale)
    for C in (1, 3, 4):
        imgs = natural_frames(2, 37, 70, C, seed=C)
        imgs[1, :, 35:] = rng.integers(0, 256, (37, 35, C), dtype=np.uint8)
        want = np.stack([c_oracle.pipeline(luts, stages, modes, scale, im, interval=interval) for im in imgs])
        assert np.array_equal(e.pipeline(dev(imgs)).cpu().numpy(), want), ("HWC", C)
        chw = np.ascontiguousarray(imgs.transpose(0, 3, 1, 2))
        got = e.pipeline(dev(chw), layout=LAYOUT_CHW).cpu().numpy().transpose(0, 2, 3, 1)
        assert np.array_equal(got, want), ("CHW", C)
    e.close()


@pytest.mark.parametrize("interval,scale,modes,route", [
    (5, 4, "sdy", "global"), (5, 4, "s", "global"), (5, 3, "sdy", "global"), (5, 3, "s", "lds"), (5, 2, "sdy", "lds"),
    (5, 2, "sdys", "global"), (5, 1, "sdysdyds", "lds"), (6, 4, "sdysdyds", "lds"), (6, 3, "sdy", "lds")])
def test_route_by_table_bytes(interval, scale, modes, route):
    """The stage's tables go to LDS when M * L^4 * row bytes fit 96 KiB, else rows are gathered from global memory."""
    luts = make_luts(2, modes, scale, interval, seed=3)
    e = engine(2, modes, scale, interval, luts)
    assert e.kernel_name(True) == "stage_interval_kernel<%d,%d,%s>" % (interval, scale, route)
    assert e.kernel_name(False) == "stage_interval_kernel<%d,1,lds>" % interval
    img = natural_noise(45, 67, 5)
    assert np.array_equal(e.pipeline(dev(img)).cpu().numpy(), c_oracle.pipeline(luts, 2, modes, scale, img, interval=interval))
    e.close()


@pytest.mark.parametrize("interval", [5, 6])
@pytest.mark.parametrize("modes", ["e", "h", "o", "eho", "sdyeho", "sdyehoeh"])
@pytest.mark.parametrize("stages,scale", [(1, 1), (2, 4), (2, 2)])
def test_wide_and_mixed_lists_match_emulator(emul_iv, interval, modes, stages, scale):  # noqa: F811
    luts = make_luts(stages, modes, scale, interval, seed=9)
    e = engine(stages, modes, scale, interval, luts)
    assert e.halo == (3 if set(modes) & set("eho") else 2) * stages
    img = natural_noise(29, 41, 2)
    assert np.array_equal(e.pipeline(dev(img)).cpu().numpy(), emul_pipeline(emul_iv, luts, stages, modes, scale, interval, img))
    e.close()


def test_batch_of_photographic_frames():
    """6 photographic 333 x 510 frames (288 tiles of 64 x 64), W % 16 != 0, H % 4 != 0: the x4 final stage on the global route, then
    x2 at interval 6.  (Persistent workgroups walking several tiles: test_persistent_workgroups_walk_several_tiles.)"""
    interval, stages, modes, scale = 5, 2, "sdy", 4
    luts = make_luts(stages, modes, scale, interval, seed=1)
    e = engine(stages, modes, scale, interval, luts)
    imgs = natural_frames(6, 333, 510, 3, seed=7)
    got = e.pipeline(dev(imgs)).cpu().numpy()
    for k in range(6):
        assert np.array_equal(got[k], c_oracle.pipeline(luts, stages, modes, scale, imgs[k], interval=interval)), k
    e.configure(stages, modes, 2, 6).set_lut_dict(make_luts(stages, modes, 2, 6, seed=1))
    luts6 = make_luts(stages, modes, 2, 6, seed=1)
    got = e.pipeline(dev(imgs[:3])).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], c_oracle.pipeline(luts6, stages, modes, 2, imgs[k], interval=6)), k
    e.close()


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("interval,modes,scale,final_route,per_cu", [
    (5, "sdy", 2, "lds", 1),           # stage 1: 1-byte rows, two workgroups per CU; final: 3 x 26 KB tables, one per CU
    (6, "sdysdyds", 4, "lds", 1)])     # final: 8 x 10 KB tables, one workgroup per CU
def test_persistent_workgroups_walk_several_tiles(interval, modes, scale, final_route, per_cu):
    """The LDS route launches at most 2 (1-byte rows) or 1 (larger tables) workgroups per CU, each walking tiles: batches of
    130 x 190 photographic frames (9 tiles each, partial tiles at the right and bottom) with more tiles than workgroups, so the tables
    staged once are reused across tiles, the tile-loop barriers guard the image tile and the tile order without the XCD remap runs."""
    stages = 2
    luts = make_luts(stages, modes, scale, interval, seed=13)
    e = engine(stages, modes, scale, interval, luts)
    assert e.kernel_name(False) == "stage_interval_kernel<%d,1,lds>" % interval
    assert e.kernel_name(True) == "stage_interval_kernel<%d,%d,%s>" % (interval, scale, final_route)
    cus = _num_cus()
    # enough frames that the stage 1 grid (two workgroups per CU) and the final one (per_cu per CU) both walk several tiles
    N = (2 * cus) // 9 + 8 if per_cu == 1 and scale == 2 else cus // 9 + 4
    tiles = N * 3 * 3
    assert tiles > per_cu * cus and (scale != 2 or tiles > 2 * cus), (tiles, cus)
    imgs = natural_frames(N, 130, 190, 3, seed=17)
    imgs[::5, 40:90] = np.random.default_rng(17).integers(0, 256, (len(imgs[::5]), 50, 190, 3), dtype=np.uint8)
    got = e.pipeline(dev(imgs)).cpu().numpy()
    for k in range(N):
        assert np.array_equal(got[k], c_oracle.pipeline(luts, stages, modes, scale, imgs[k], interval=interval)), k
    e.close()


@pytest.fixture(scope="module")
def frame1080():
    natural = natural_frames(1, 1080, 1920, 3, seed=11)[0]
    noise = np.random.default_rng(11).integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    return natural, noise


def test_1080p_frames_interval5(frame1080):
    interval, stages, modes, scale = 5, 2, "sdy", 4
    luts = make_luts(stages, modes, scale, interval, seed=2)
    e = engine(stages, modes, scale, interval, luts)
    for img in frame1080:
        assert np.array_equal(e.pipeline(dev(img)).cpu().numpy(), c_oracle.pipeline(luts, stages, modes, scale, img, interval=interval))
    e.close()


@pytest.mark.parametrize("band", [135, 270])
def test_strips_equal_the_whole_frame(frame1080, band):
    for interval, modes in ((5, "sdy"), (6, "sdyo")):
        stages, scale = 2, 4
        e = engine(stages, modes, scale, interval, make_luts(stages, modes, scale, interval, seed=4))
        img = frame1080[0].copy()
        img[500:700] = frame1080[1][500:700]
        H = img.shape[0]
        full = e.pipeline(dev(img))
        halo = e.halo
        parts = []
        for y0 in range(0, H, band):
            y1 = min(H, y0 + band)
            r0, r1 = max(0, y0 - halo), min(H, y1 + halo)
            parts.append(e.pipeline_rows(dev(img[r0:r1]), r0, y0, y1, H))
        assert torch.equal(torch.cat(parts, 0), full), (interval, band)
        e.close()


@pytest.mark.parametrize("interval,stages,modes,scale", [(5, 2, "sdy", 4), (6, 3, "sdyeho", 2), (5, 1, "o", 3)])
def test_pipeline_replays_from_a_captured_graph(interval, stages, modes, scale):
    e = engine(stages, modes, scale, interval, make_luts(stages, modes, scale, interval, seed=8))
    img = np.random.default_rng(3).integers(0, 256, (2, 45, 77, 3), dtype=np.uint8)
    img[0, :, :38] = natural_frames(1, 45, 38, 3, seed=4)[0]
    x = dev(img)
    out = torch.empty((2, 45 * scale, 77 * scale, 3), dtype=torch.uint8, device="cuda")
    e.reserve(2, 45, 77, 3)                       # no allocation inside the captured region
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        e.pipeline(x, out=out)                    # warm-up: kernel attributes are set on first launch
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e.pipeline(x, out=out)
    for trial in range(2):
        x.copy_(dev(np.roll(img, trial, axis=2)))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = e.pipeline(x).clone()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), trial
    e.close()


def test_reconfigure_4_5_6_4(shipped_luts):
    img = natural_noise(40, 90, 3)
    stages, modes, scale = 2, "sdy", 4
    e = MuLUTEngine(0)
    for interval in (4, 5, 6, 4):
        luts = shipped_luts if interval == 4 else make_luts(stages, modes, scale, interval, seed=interval)
        e.configure(stages, modes, scale, interval)
        with pytest.raises(MuLUTError, match="not set"):       # another interval's tables were cleared (none at all at first)
            e.pipeline(dev(img))
        e.set_lut_dict(luts)
        got = e.pipeline(dev(img)).cpu().numpy()
        fresh = engine(stages, modes, scale, interval, luts)
        assert np.array_equal(got, fresh.pipeline(dev(img)).cpu().numpy()), interval
        fresh.close()
        assert np.array_equal(got, c_oracle.pipeline(luts, stages, modes, scale, img, interval=interval)), interval
    e.close()


@pytest.mark.parametrize("interval", [5, 6])
def test_tuning_keys_do_not_change_the_interval_route(interval):
    stages, modes, scale = 2, "sdy", 4
    luts = make_luts(stages, modes, scale, interval, seed=6)
    img = natural_noise(40, 70, 6)
    base = engine(stages, modes, scale, interval, luts)
    want, names = base.pipeline(dev(img)).cpu().numpy(), (base.kernel_name(False), base.kernel_name(True))
    base.close()
    for key, value in (("first_stage_kernel", 2), ("first_stage_kernel", 3), ("final_stage_kernel", 1), ("final_stage_kernel", 5),
                       ("tube_pipelined", 0), ("detail_kernel", 1), ("stat_from_first_stage", 0), ("hybrid_oob_per_1024", 0),
                       ("first_stage_detail_per_1024", 0), ("final_stage_detail_per_1024", 1024)):
        e = engine(stages, modes, scale, interval, luts)
        e.set_tuning(key, value)
        assert np.array_equal(e.pipeline(dev(img)).cpu().numpy(), want), (key, value)
        assert (e.kernel_name(False), e.kernel_name(True)) == names, (key, value)
        e.close()


# ---------------------------------------------------------------------------------------------
# the command-line twin on Set5 with tables transferred from the shipped network, under the writers' names
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", [5, 6])
def test_cli_set5_with_reference_tables(ivfx, tmp_path, capsys, interval):  # noqa: F811
    """The tables the reference's transfer made, under the writers' {interval}bit names, through the CLI twin with --lutName LUT:
    the HR pixels of every Set5 image and the summary line are the reference's (gen_golden_interval.py)."""
    import hashlib
    from mulut_amd import test_lut
    stages, modes, scale = 2, "sdy", 4
    exp = tmp_path / "models" / "sr_iv"
    exp.mkdir(parents=True)
    for key, t in fixture_luts(ivfx, interval).items():
        np.save(str(exp / ("LUT_x4_%dbit_int8_%s.npy" % (interval, key))), t.reshape(t.shape[0], 1, *(2 * (int(np.sqrt(t.shape[1])),))))
    test_dir = tmp_path / "SRBenchmark"
    (test_dir / "Set5").mkdir(parents=True)
    os.symlink(os.path.join(GOLDEN, "Set5", "HR"), test_dir / "Set5" / "HR")
    os.symlink(os.path.join(GOLDEN, "Set5", "LR_bicubic"), test_dir / "Set5" / "LR_bicubic")
    capsys.readouterr()
    res = test_lut.main(["--stages", str(stages), "--modes", modes, "-e", str(exp), "--testDir", str(test_dir),
                         "--resultRoot", str(tmp_path / "results"), "--lutName", "LUT", "--interval", str(interval)])
    assert res["Set5"].shape == (5, 2)
    assert str(ivfx["iv%d/set5/summary" % interval]) in capsys.readouterr().out.splitlines()
    out_dir = tmp_path / "results" / "sr_iv" / "Set5" / "X4"
    files = sorted(os.listdir(os.path.join(GOLDEN, "Set5", "HR")))
    assert len(files) == 5
    for fn in files:
        px = np.ascontiguousarray(np.array(Image.open(out_dir / ("%s_LUT_%dbit.png" % (fn[:-4], 8 - interval)))))
        assert hashlib.sha256(px.tobytes()).hexdigest() == str(ivfx["iv%d/set5/%s/sha256" % (interval, fn[:-4])]), fn


def test_finetune_module_refuses_interval_5(tmp_path):
    from mulut_amd.finetune import MuLUT
    with pytest.raises(NotImplementedError, match="interval-4 only"):
        MuLUT(str(tmp_path), 2, "sdy", upscale=4, interval=5)
