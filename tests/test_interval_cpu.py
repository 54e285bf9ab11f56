"""Sampling intervals 5 and 6 on the CPU: the per-site math of mulut_interval.h (tests/host_emul/emul_interval.cpp, g++) against the
C oracle and the NumPy port at those intervals, and the table-file rules of lut_io (reader's ``{8-interval}bit`` name first, then the
writers' ``{interval}bit``, taken only with the interval's L^4 rows).  oracle/np_port.py takes its pattern table from module-level
dicts; e, h, o are added to them here for the test only."""
import ctypes
import os

import numpy as np
import pytest

from host_emul_lib import load_emul
from oracle import c_oracle, np_port

from mulut_amd import lut_io

WIDE_PATTERNS = {"e": ((0, 0), (0, 3), (3, 0), (3, 3)), "h": ((0, 0), (2, 2), (2, 3), (3, 2)), "o": ((0, 0), (2, 2), (1, 3), (3, 1))}


@pytest.fixture(scope="module")
def emul_iv():
    L = load_emul("emul_interval", ["mulut_core.h", "mulut_interval.h"])
    L.emul_stage_interval.restype = ctypes.c_int
    L.emul_check_rhe_interval.restype = ctypes.c_long
    return L


@pytest.fixture
def np_wide(monkeypatch):
    for m, taps in WIDE_PATTERNS.items():
        monkeypatch.setitem(np_port.PATTERNS, m, taps)
        monkeypatch.setitem(np_port.PAD, m, 3)
    return np_port


def run_emul_iv(L, luts, modes, is_last, img_hwc, u, interval):
    img = np.ascontiguousarray(img_hwc.transpose(2, 0, 1))
    C, H, W = img.shape
    keep = [np.ascontiguousarray(t, dtype=np.int8) for t in luts]
    arr = (ctypes.c_void_p * len(keep))(*[t.ctypes.data for t in keep])
    out = np.empty((H * u, W * u, C), np.uint8)
    rc = L.emul_stage_interval(arr, modes.encode(), len(modes), int(is_last), ctypes.c_void_p(img.ctypes.data), H, W, C, u,
                               interval, ctypes.c_void_p(out.ctypes.data))
    assert rc == 0
    return out


def _tables(rng, modes, u, interval):
    return {m: rng.integers(-128, 128, (lut_io.lut_rows(interval), u * u), dtype=np.int8) for m in set(modes)}   # includes -128


@pytest.mark.parametrize("interval", [5, 6])
def test_rhe_epilogue_exhaustive(emul_iv, interval):
    assert emul_iv.emul_check_rhe_interval(interval) == 0


@pytest.mark.parametrize("interval", [5, 6])
@pytest.mark.parametrize("u", [1, 2, 3, 4])
@pytest.mark.parametrize("modes", ["s", "d", "y", "sdy", "yds"])
def test_emulator_matches_oracle_stage(emul_iv, interval, u, modes):
    rng = np.random.default_rng(100 * interval + 10 * u + len(modes))
    tabs = _tables(rng, modes, u, interval)
    luts = [tabs[m] for m in modes]
    for H, W, C in ((1, 1, 1), (2, 7, 1), (9, 14, 3), (5, 3, 2)):
        img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        for last in (True, False):
            got = run_emul_iv(emul_iv, luts, modes, last, img, u, interval)
            want = c_oracle.stage(luts, modes, last, img, u, interval=interval)
            assert np.array_equal(got, want), (interval, u, modes, (H, W, C), last)


@pytest.mark.parametrize("interval", [5, 6])
def test_emulator_extremes_and_grid_vertices(emul_iv, interval):
    """Values on the sampling grid (weights concentrate on one vertex), 0 / 255 (the top cell) and saturated tables (clip)."""
    q = 2 ** interval
    rng = np.random.default_rng(interval)
    grid = np.array([0, q, 2 * q, 255 - q, 254, 255, q - 1, q + 1], np.uint8)
    img = grid[rng.integers(0, len(grid), (11, 13, 3))]
    for val in (127, -128, None):
        for u, last in ((1, False), (1, True), (4, True), (3, True)):
            rows = lut_io.lut_rows(interval)
            luts = [np.full((rows, u * u), val, np.int8) if val is not None else rng.integers(-128, 128, (rows, u * u), dtype=np.int8)
                    for _ in "sdy"]
            assert np.array_equal(run_emul_iv(emul_iv, luts, "sdy", last, img, u, interval),
                                  c_oracle.stage(luts, "sdy", last, img, u, interval=interval)), (val, u, last)


@pytest.mark.parametrize("interval", [5, 6])
@pytest.mark.parametrize("stages,scale", [(1, 4), (2, 4), (3, 2), (2, 1)])
def test_emulator_cascade_matches_oracle_pipeline(emul_iv, interval, stages, scale):
    rng = np.random.default_rng(stages * 10 + scale + interval)
    modes = "sdy"
    luts = {"s%d_%s" % (s + 1, m): rng.integers(-127, 128, (lut_io.lut_rows(interval), scale * scale if s + 1 == stages else 1),
                                                 dtype=np.int8) for s in range(stages) for m in modes}
    img = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    cur = img
    for s in range(stages):
        last = s + 1 == stages
        cur = run_emul_iv(emul_iv, [luts["s%d_%s" % (s + 1, m)] for m in modes], modes, last, cur, scale if last else 1, interval)
    assert np.array_equal(cur, c_oracle.pipeline(luts, stages, modes, scale, img, interval=interval))


def _np_stage(tabs, modes, is_last, img, u, interval):
    """One stage of np_port.run_stages (the reference's loop) with the given tables."""
    lut = {"s1_" + m: t.astype(np.float32) for m, t in tabs.items()}
    if is_last:
        return np_port.run_stages(lut, 1, modes, u, img, interval=interval)
    lut.update({"s2_" + m: np.zeros((lut_io.lut_rows(interval), 1), np.float32) for m in tabs})
    return np_port.run_stages(lut, 2, modes, 1, img, interval=interval, return_all=True)[0]


@pytest.mark.parametrize("interval", [5, 6])
@pytest.mark.parametrize("modes", ["e", "h", "o", "eho", "sdyeho", "sdyehoeh"])
@pytest.mark.parametrize("u,is_last", [(1, False), (1, True), (2, True), (4, True)])
def test_emulator_matches_np_port_wide(emul_iv, np_wide, interval, modes, u, is_last):
    rng = np.random.default_rng(interval * 100 + len(modes) * 10 + u)
    img = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    img[:4, :5] = img[0, 0] // 2 ** interval * 2 ** interval      # a flat grid-aligned patch
    tabs = _tables(rng, modes, u, interval)
    got = run_emul_iv(emul_iv, [tabs[m] for m in modes], modes, is_last, img, u, interval)
    assert np.array_equal(got, _np_stage(tabs, modes, is_last, img, u, interval)), (interval, modes, u, is_last)


@pytest.mark.parametrize("interval", [5, 6])
def test_emulator_matches_np_port_sdy(emul_iv, interval):
    rng = np.random.default_rng(interval)
    img = rng.integers(0, 256, (7, 10, 2), dtype=np.uint8)
    for u, last in ((1, False), (3, True)):
        tabs = _tables(rng, "sdy", u, interval)
        assert np.array_equal(run_emul_iv(emul_iv, [tabs[m] for m in "sdy"], "sdy", last, img, u, interval),
                              _np_stage(tabs, "sdy", last, img, u, interval))


# ---- table files --------------------------------------------------------------------------------------------------------------
def _write(d, name, arr):
    np.save(os.path.join(str(d), name), arr)


def test_lut_rows():
    assert [lut_io.lut_rows(i) for i in (4, 5, 6)] == [83521, 6561, 625]
    assert lut_io.L_ROWS == lut_io.lut_rows(4)


@pytest.mark.parametrize("interval", [5, 6])
def test_load_reader_name_first_then_writer_name(tmp_path, interval):
    rows = lut_io.lut_rows(interval)
    rng = np.random.default_rng(interval)
    reader = {(s, m): rng.integers(-127, 128, (rows, 16 if s == 2 else 1), dtype=np.int8) for s in (1, 2) for m in "sdy"}
    writer = {k: (v.astype(np.int16) // 2).astype(np.int8) for k, v in reader.items()}
    # writer names only (what the reference's transfer / fine-tune scripts leave behind)
    for (s, m), t in writer.items():
        _write(tmp_path, "LUT_x4_{}bit_int8_s{}_{}.npy".format(interval, s, m), t)
    got = lut_io.load_lut_dict(str(tmp_path), 2, "sdy", 4, interval, "LUT")
    assert all(np.array_equal(got["s%d_%s" % k], v) for k, v in writer.items())
    # the reader's name, when present with the right rows, wins
    for (s, m), t in reader.items():
        _write(tmp_path, "LUT_x4_{}bit_int8_s{}_{}.npy".format(8 - interval, s, m), t)
    got = lut_io.load_lut_dict(str(tmp_path), 2, "sdy", 4, interval, "LUT")
    assert all(np.array_equal(got["s%d_%s" % k], v) for k, v in reader.items())
    assert got["s2_s"].shape == (rows, 16) and got["s1_d"].shape == (rows, 1)
    # (L^4, 1, u, u) files load as (L^4, u*u)
    _write(tmp_path, "LUT_x4_{}bit_int8_s2_y.npy".format(8 - interval), reader[(2, "y")].reshape(rows, 1, 4, 4))
    assert lut_io.load_lut_dict(str(tmp_path), 2, "sdy", 4, interval, "LUT")["s2_y"].shape == (rows, 16)


def test_interval5_skips_interval3_table_of_the_same_name(tmp_path):
    """'3bit' is the reader's name at interval 5 AND the writers' name at interval 3 (33^4 rows): only the row count tells them apart."""
    t5 = np.random.default_rng(0).integers(-127, 128, (6561, 1), dtype=np.int8)
    _write(tmp_path, "LUT_x1_3bit_int8_s1_s.npy", np.zeros((33 ** 4, 1), np.int8))
    _write(tmp_path, "LUT_x1_5bit_int8_s1_s.npy", t5)
    got = lut_io.load_lut_dict(str(tmp_path), 1, "s", 1, 5, "LUT")
    assert np.array_equal(got["s1_s"], t5)
    os.remove(os.path.join(str(tmp_path), "LUT_x1_5bit_int8_s1_s.npy"))
    with pytest.raises(FileNotFoundError, match="LUT_x1_3bit_int8_s1_s.npy and LUT_x1_5bit_int8_s1_s.npy"):
        lut_io.load_lut_dict(str(tmp_path), 1, "s", 1, 5, "LUT")


@pytest.mark.parametrize("interval", [5, 6])
def test_missing_table_names_both_candidates(tmp_path, interval):
    with pytest.raises(FileNotFoundError) as ei:
        lut_io.load_lut_dict(str(tmp_path), 1, "d", 2, interval, "LUT_ft")
    msg = str(ei.value)
    assert "LUT_ft_x2_{}bit_int8_s1_d.npy".format(8 - interval) in msg
    assert "LUT_ft_x2_{}bit_int8_s1_d.npy".format(interval) in msg


def test_interval4_names_and_arrays_unchanged(tmp_path):
    from conftest import GOLDEN
    assert lut_io.lut_file_name("LUT_ft", 4, 4, 1, "s") == "LUT_ft_x4_4bit_int8_s1_s.npy"
    assert lut_io.writer_file_name("LUT", 4, 4, 2, "y") == "LUT_x4_4bit_int8_s2_y.npy"
    got = lut_io.load_lut_dict(os.path.join(GOLDEN, "luts"), 2, "sdy", 4, 4, "LUT_ft")
    for s in (1, 2):
        for m in "sdy":
            raw = np.load(os.path.join(GOLDEN, "luts", "LUT_ft_x4_4bit_int8_s%d_%s.npy" % (s, m)))
            assert np.array_equal(got["s%d_%s" % (s, m)], raw.reshape(83521, -1))
    with pytest.raises(FileNotFoundError):
        lut_io.load_lut_dict(str(tmp_path), 1, "s", 4, 4, "LUT_ft")
    # interval 4 never falls back to another name: a 6561-row file there is a shape error, as before
    _write(tmp_path, "LUT_ft_x1_4bit_int8_s1_s.npy", np.zeros((6561, 1), np.int8))
    with pytest.raises(ValueError):
        lut_io.load_lut_dict(str(tmp_path), 1, "s", 1, 4, "LUT_ft")


def test_synthetic_lut_default_unchanged():
    a = lut_io.synthetic_lut(7, 16)
    rng = np.random.default_rng(7)
    assert np.array_equal(a, rng.integers(-127, 128, size=(83521, 16), dtype=np.int8))
    assert lut_io.synthetic_lut(7, 1, interval=5).shape == (6561, 1)
    assert lut_io.synthetic_lut(7, 4, interval=6).shape == (625, 4)


@pytest.mark.parametrize("interval", [5, 6])
def test_transfer_grid_and_names(interval):
    """The producer's grid is arange(0, 257, 2^interval) with 256 -> 255 (sr/2_transfer_to_lut.py:14-15), L^4 rows, a slowest;
    its file name is the writers' {interval}bit one."""
    from types import SimpleNamespace
    from mulut_amd import transfer_to_lut as T
    opt = SimpleNamespace(stages=2, modes="sdy", scale=4, interval=interval, expDir="")
    x = T.get_input_tensor(opt)
    L = 2 ** (8 - interval) + 1
    assert x.shape == (L ** 4, 1, 2, 2)
    base = np.minimum(np.arange(0, 257, 2 ** interval), 255)
    v = np.round(x.numpy() * 255).astype(int).reshape(-1, 4)
    assert np.array_equal(v[:, 0], np.repeat(base, L ** 3)) and np.array_equal(v[:, 3], np.tile(base, L ** 3))
    assert T.lut_file_name(opt, 1, "s") == "LUT_x4_{}bit_int8_s1_s.npy".format(interval)


# ---- anchored to the reference (tests/golden/interval_fixtures.npz, gen_golden_interval.py) -------------------------------------
@pytest.fixture(scope="module")
def ivfx():
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "interval_fixtures.npz"))


def fixture_luts(fx, interval):
    return {k.split("/")[-1]: fx[k] for k in fx.files if k.startswith("iv%d/lut/" % interval)}


def fixture_passes(fx, interval):
    """(input name, u, mode, r, sha256, array or None) of every recorded reference pass"""
    out = []
    for k in fx.files:
        parts = k.split("/")
        if parts[0] == "iv%d" % interval and parts[1] == "pass" and parts[-1] == "sha256":
            name, u, mode, r = parts[2], int(parts[3][1:]), parts[4], int(parts[5][1:])
            arr = fx[k[:-len("sha256")] + "q"] if (k[:-len("sha256")] + "q") in fx.files else None
            out.append((name, u, mode, r, str(fx[k]), arr))
    return out


def sha256_i32(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


@pytest.mark.parametrize("interval", [5, 6])
def test_oracle_pass_matches_reference_fixtures(ivfx, interval):
    luts = fixture_luts(ivfx, interval)
    cases = fixture_passes(ivfx, interval)
    assert len(cases) == 6 * 2 * 3 * 4
    for name, u, mode, r, sha, arr in cases:
        img = np.ascontiguousarray(ivfx["iv%d/in/%s" % (interval, name)].transpose(2, 0, 1))
        got = c_oracle.pass_q(luts["s%d_%s" % (1 if u == 1 else 2, mode)], img, r, u, mode, interval=interval)
        if arr is not None:
            assert np.array_equal(got, arr), (name, u, mode, r)
        assert sha256_i32(got) == sha, (name, u, mode, r)


@pytest.mark.parametrize("interval", [5, 6])
def test_emulator_cascade_matches_reference_crop(emul_iv, ivfx, interval):
    import hashlib
    luts = fixture_luts(ivfx, interval)
    img = ivfx["in/crop"]
    s1 = run_emul_iv(emul_iv, [luts["s1_" + m] for m in "sdy"], "sdy", False, img, 1, interval)
    assert np.array_equal(s1, ivfx["iv%d/crop/stage1" % interval])
    fin = run_emul_iv(emul_iv, [luts["s2_" + m] for m in "sdy"], "sdy", True, s1, 4, interval)
    assert hashlib.sha256(np.ascontiguousarray(fin).tobytes()).hexdigest() == str(ivfx["iv%d/crop/final_sha256" % interval])


@pytest.mark.parametrize("interval", [5, 6])
def test_transfer_matches_reference_tables(ivfx, interval):
    """transfer_to_lut on the shipped checkpoint at interval 5 / 6 against the tables the reference's transfer made: at most 1 LSB
    apart on at most 0.01 % of the entries (the tolerance of the interval-4 transfer test)."""
    from types import SimpleNamespace
    from conftest import GOLDEN
    from mulut_amd import network, transfer_to_lut as T
    net = network.SRNets(nf=64, scale=4, modes=list("sdy"), stages=2)
    net.load_state_dict(network.load_checkpoint(os.path.join(GOLDEN, "Model_200000.pth")).state_dict(), strict=True)
    opt = SimpleNamespace(stages=2, modes="sdy", scale=4, interval=interval, expDir="")
    got = T.transfer(net, opt, save=False)
    want = fixture_luts(ivfx, interval)
    assert sorted(got) == sorted(want)
    for k, t in got.items():
        t = t.reshape(t.shape[0], -1)
        assert t.shape == want[k].shape == (lut_io.lut_rows(interval), 16 if k.startswith("s2") else 1), k
        diff = np.abs(t.astype(np.int16) - want[k].astype(np.int16))
        assert diff.max() <= 1 and (diff > 0).mean() <= 1e-4, (k, int(diff.max()), float((diff > 0).mean()))


@pytest.mark.parametrize("interval", [5, 6])
def test_oracle_and_metrics_reproduce_reference_set5(ivfx, interval):
    """The C oracle with the reference-made tables gives the reference's Set5 x4 pixels, and the metrics restatement its summary line."""
    import hashlib
    from PIL import Image
    from conftest import GOLDEN
    from mulut_amd.metrics import modcrop, psnr, rgb2ycbcr, ssim
    luts = fixture_luts(ivfx, interval)
    ps = []
    for fn in sorted(os.listdir(os.path.join(GOLDEN, "Set5", "HR"))):
        lr = np.array(Image.open(os.path.join(GOLDEN, "Set5", "LR_bicubic", "X4", fn)))
        lr = np.stack([lr] * 3, axis=2) if lr.ndim == 2 else lr
        out = c_oracle.pipeline(luts, 2, "sdy", 4, lr, interval=interval)
        assert hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest() == str(ivfx["iv%d/set5/%s/sha256" % (interval, fn[:-4])]), fn
        gt = modcrop(np.array(Image.open(os.path.join(GOLDEN, "Set5", "HR", fn))), 4)
        gt = np.stack([gt] * 3, axis=2) if gt.ndim == 2 else gt
        y0, y1 = rgb2ycbcr(gt)[:, :, 0], rgb2ycbcr(out)[:, :, 0]
        ps.append((psnr(y0, y1, 4), ssim(y0, y1)))
    ps = np.asarray(ps)
    line = "Dataset Set5 | AVG LUT PSNR: {:.2f} SSIM: {:.4f}".format(np.mean(ps[:, 0]), np.mean(ps[:, 1]))
    assert line == str(ivfx["iv%d/set5/summary" % interval])
