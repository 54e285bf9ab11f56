"""The 4 x 4 sampling patterns e, h, o on the GPU (-m gpu): mode lists that hold one of them ("wide" lists, reach 3 per stage) run
every stage on the 3-px-halo instances of stage_u1w_kernel (mulut_k1.hip) and stage_up_kernel (mulut_kernels.hip).  Checked bit-exactly against the host emulator of mulut_core.h
(tests/host_emul) and against the NumPy port of the reference's loop with e, h, o added to its pattern table for the test."""
import ctypes
import os

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN
from oracle import np_port
from test_core_math_cpu import emul, run_emul  # noqa: F401  (the host emulator fixture and driver)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine, MuLUTError, synthetic_lut  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402

WIDE_PATTERNS = {"e": ((0, 0), (0, 3), (3, 0), (3, 3)), "h": ((0, 0), (2, 2), (2, 3), (3, 2)), "o": ((0, 0), (2, 2), (1, 3), (3, 1))}
MODE_LISTS = ["e", "h", "o", "eho", "sdyeho", "sdyehoeh"]


@pytest.fixture
def np_wide(monkeypatch):
    for m, taps in WIDE_PATTERNS.items():
        monkeypatch.setitem(np_port.PATTERNS, m, taps)
        monkeypatch.setitem(np_port.PAD, m, 3)
    return np_port


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def make_luts(stages, modes, scale, seed=0):
    return {"s%d_%s" % (s + 1, m): synthetic_lut(seed + 31 * s + ord(m), scale * scale if s + 1 == stages else 1)
            for s in range(stages) for m in modes}


def emul_pipeline(L, luts, stages, modes, scale, img_hwc):
    """The cascade on the host emulator, channel by channel (channels are independent planes)."""
    outs = []
    for c in range(img_hwc.shape[2]):
        cur = np.ascontiguousarray(img_hwc[:, :, c:c + 1])
        for s in range(stages):
            last = s + 1 == stages
            cur = run_emul(L, [luts["s%d_%s" % (s + 1, m)] for m in modes], modes, last, cur, scale if last else 1)
        outs.append(cur)
    return np.concatenate(outs, axis=2)


def engine(stages, modes, scale, luts):
    return MuLUTEngine(0).configure(stages, modes, scale, 4).set_lut_dict(luts)


# ---------------------------------------------------------------------------------------------
# one pass: mulut_pass and the FourSimplexInterpFaster twin against the extended NumPy port
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u", [1, 2, 3, 4])
def test_pass_all_rotations(np_wide, u):
    from mulut_amd.interp import FourSimplexInterpFaster
    img = np.random.default_rng(u).integers(0, 256, (13, 10, 2), dtype=np.uint8)
    img[:5, :6] = 96                                             # grid-aligned flat patch
    for m in "eho":
        table = synthetic_lut(ord(m) + u, u * u)
        e = MuLUTEngine(0).configure(1, m, u, 4)
        e.set_lut(1, m, table)
        for r in range(4):
            rimg = np.rot90(img, r)
            h, w, _ = rimg.shape
            img_in = np.pad(rimg, ((0, 3), (0, 3), (0, 0)), mode="edge").transpose(2, 0, 1).astype(np.float32)
            want = np_wide.four_simplex_interp(table.astype(np.float32), img_in, h, w, 4, 4 - r, upscale=u, mode=m)
            got = e.pass_q(1, m, r, dev(img.transpose(2, 0, 1))).cpu().numpy()
            assert np.array_equal(got, np.rint(want * 16).astype(np.int64)), (m, u, r)
            twin = FourSimplexInterpFaster(table.astype(np.float32), img_in, h, w, 4, 4 - r, upscale=u, mode=m)
            assert twin.dtype == np.float64 and np.array_equal(twin, want), (m, u, r)
        e.close()


# ---------------------------------------------------------------------------------------------
# whole cascades against the emulator (and, small ones, against the NumPy port directly)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modes", MODE_LISTS)
@pytest.mark.parametrize("stages,scale", [(1, 1), (1, 3), (2, 4), (3, 2)])
def test_pipeline_vs_emulator(emul, modes, stages, scale):  # noqa: F811
    luts = make_luts(stages, modes, scale, seed=len(modes))
    e = engine(stages, modes, scale, luts)
    rng = np.random.default_rng(stages * 10 + scale)
    nat = natural_frames(1, 37, 45, 4, seed=scale)[0]           # W % 16 != 0, H % 4 != 0
    noisy = rng.integers(0, 256, (37, 45, 4), dtype=np.uint8)
    for C in (1, 3, 4):
        img = np.stack([nat[:, :, :C], noisy[:, :, :C]])
        want = np.stack([emul_pipeline(emul, luts, stages, modes, scale, im) for im in img])
        got = e.pipeline(dev(img)).cpu().numpy()
        assert np.array_equal(got, want), (modes, stages, scale, C, "HWC")
        got = e.pipeline(dev(img.transpose(0, 3, 1, 2)), layout=LAYOUT_CHW).cpu().numpy()
        assert np.array_equal(got, want.transpose(0, 3, 1, 2)), (modes, stages, scale, C, "CHW")
    one = rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)       # 1 x 1
    assert np.array_equal(e.pipeline(dev(one)).cpu().numpy(), emul_pipeline(emul, luts, stages, modes, scale, one))
    e.close()


@pytest.mark.parametrize("modes,stages,scale", [("eho", 2, 4), ("sdyeho", 2, 2), ("oh", 1, 3), ("e", 3, 1)])
def test_small_pipeline_vs_np_port(np_wide, modes, stages, scale):
    luts = make_luts(stages, modes, scale, seed=5)
    img = np.random.default_rng(9).integers(0, 256, (11, 14, 3), dtype=np.uint8)
    e = engine(stages, modes, scale, luts)
    want = np_wide.run_stages({k: v.astype(np.float32) for k, v in luts.items()}, stages, modes, scale, img)
    assert np.array_equal(e.pipeline(dev(img)).cpu().numpy(), want)
    e.close()


def test_batch_with_more_tiles_than_cus(emul):  # noqa: F811
    modes, stages, scale = "sdyeho", 2, 4
    luts = make_luts(stages, modes, scale, seed=2)
    e = engine(stages, modes, scale, luts)
    img = natural_frames(4, 270, 500, 3, seed=1)
    got = e.pipeline(dev(img)).cpu().numpy()
    for n in range(4):
        assert np.array_equal(got[n], emul_pipeline(emul, luts, stages, modes, scale, img[n])), n
    assert "wide" in e.kernel_name(True) and "wide" in e.kernel_name(False)
    e.close()


# ---------------------------------------------------------------------------------------------
# halo, strips, graph capture
# ---------------------------------------------------------------------------------------------
def test_halo_is_three_per_stage_for_wide_lists():
    for stages in (1, 2, 3):
        for modes, reach in (("sdy", 2), ("s", 2), ("eho", 3), ("sdyo", 3), ("he", 3)):
            e = MuLUTEngine(0).configure(stages, modes, 2, 4)
            assert e.halo == reach * stages, (stages, modes)
            e.close()


@pytest.mark.parametrize("nstrips", [2, 3, 8])
def test_strips_tile_bit_exactly(nstrips):
    stages, modes, scale = 2, "sdyeho", 4
    e = engine(stages, modes, scale, make_luts(stages, modes, scale, seed=4))
    H, W = 97, 61
    img = natural_frames(1, H, W, 3, seed=4)[0]
    img[40:60] = np.random.default_rng(4).integers(0, 256, (20, W, 3), dtype=np.uint8)
    full = e.pipeline(dev(img))
    halo = e.halo
    assert halo == 6
    bounds = np.linspace(0, H, nstrips + 1).astype(int)
    parts = []
    for k in range(nstrips):
        y0, y1 = int(bounds[k]), int(bounds[k + 1])
        r0, r1 = max(0, y0 - halo), min(H, y1 + halo)
        parts.append(e.pipeline_rows(dev(img[r0:r1]), r0, y0, y1, H))
    assert torch.equal(torch.cat(parts, 0), full)
    with pytest.raises(MuLUTError, match="halo"):               # band one row short of the halo
        e.pipeline_rows(dev(img[30 - halo + 1:60 + halo]), 30 - halo + 1, 30, 60, H)
    e.close()


@pytest.mark.parametrize("stages,modes,scale", [(2, "eho", 4), (3, "sdyehoeh", 2), (1, "o", 3)])
def test_pipeline_replays_from_a_captured_graph(stages, modes, scale):
    e = engine(stages, modes, scale, make_luts(stages, modes, scale, seed=8))
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


# ---------------------------------------------------------------------------------------------
# the command-line twin on Set5 with synthetic e / h / o tables
# ---------------------------------------------------------------------------------------------
def test_cli_set5_with_wide_tables(emul, tmp_path, capsys):  # noqa: F811
    from mulut_amd import test_lut
    stages, modes, scale = 2, "sdyeho", 4
    test_dir = tmp_path / "SRBenchmark"
    (test_dir / "Set5").mkdir(parents=True)
    os.symlink(os.path.join(GOLDEN, "Set5", "HR"), test_dir / "Set5" / "HR")
    os.symlink(os.path.join(GOLDEN, "Set5", "LR_bicubic"), test_dir / "Set5" / "LR_bicubic")
    exp = tmp_path / "models" / "sr_wide"
    exp.mkdir(parents=True)
    luts = make_luts(stages, modes, scale, seed=12)
    for key, t in luts.items():
        s, m = key[1:].split("_")
        np.save(str(exp / ("LUT_x4_4bit_int8_s%s_%s.npy" % (s, m))), t.reshape(-1, 1, *(2 * (int(np.sqrt(t.shape[1])),))))
    res = test_lut.main(["--stages", str(stages), "--modes", modes, "-e", str(exp), "--testDir", str(test_dir),
                         "--resultRoot", str(tmp_path / "results"), "--lutName", "LUT"])
    assert res["Set5"].shape == (5, 2)
    out_dir = tmp_path / "results" / "sr_wide" / "Set5" / "X4"
    files = sorted(os.listdir(os.path.join(GOLDEN, "Set5", "LR_bicubic", "X4")))
    assert len(files) == 5
    for fn in files:
        lr = np.array(Image.open(os.path.join(GOLDEN, "Set5", "LR_bicubic", "X4", fn)))
        if lr.ndim == 2:
            lr = np.stack([lr] * 3, axis=2)
        want = emul_pipeline(emul, luts, stages, modes, scale, lr)
        got = np.array(Image.open(out_dir / ("%s_LUT_4bit.png" % fn[:-4])))
        assert np.array_equal(got, want), fn


# ---------------------------------------------------------------------------------------------
# fine-tuning stays with s, d, y
# ---------------------------------------------------------------------------------------------
def test_finetune_refuses_wide_modes(tmp_path):
    from mulut_amd import _native
    from mulut_amd.finetune import MuLUT
    lib = _native.load()
    w = torch.zeros((17 ** 4, 1), dtype=torch.float32, device="cuda")
    x = torch.zeros((1, 1, 8, 8), dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    ptrs = (ctypes.c_void_p * 1)(w.data_ptr())
    for m in "eho":
        rc = lib.mulut_ft_stage_forward(0, ptrs, m.encode(), 0, 1, x.data_ptr(), 1, 1, 8, 8, out.data_ptr(), None)
        assert rc == -2, m                                       # MULUT_EMODE
    rc = lib.mulut_ft_stage_forward(0, ptrs, b"s", 0, 1, x.data_ptr(), 1, 1, 8, 8, out.data_ptr(), None)
    assert rc == 0
    with pytest.raises(ValueError, match="Mode e not implemented"):
        MuLUT(str(tmp_path), 2, "sde", upscale=4)


def test_tuning_keys_do_not_change_the_wide_route(emul):  # noqa: F811
    stages, modes, scale = 2, "eho", 4
    luts = make_luts(stages, modes, scale, seed=6)
    img = natural_frames(1, 40, 70, 3, seed=6)[0]
    want = emul_pipeline(emul, luts, stages, modes, scale, img)
    for key, value in (("first_stage_kernel", 2), ("first_stage_kernel", 3), ("final_stage_kernel", 1), ("final_stage_kernel", 5),
                       ("tube_pipelined", 0), ("detail_kernel", 1)):
        e = engine(stages, modes, scale, luts)
        e.set_tuning(key, value)
        assert np.array_equal(e.pipeline(dev(img)).cpu().numpy(), want), (key, value)
        e.close()
