"""Host-side evaluation helpers (mulut_amd/metrics.py) against values produced by the reference's common/utils.py
(tests/golden/metrics_fixtures.npz, written by tests/golden/gen_golden_metrics.py)."""
import os

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN
from eval_pairs import big_pairs

from mulut_amd.metrics import modcrop, psnr, rgb2ycbcr, ssim


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "metrics_fixtures.npz"))


def _score(gt, out, shave):
    y_gt, y_out = rgb2ycbcr(gt)[:, :, 0], rgb2ycbcr(out)[:, :, 0]
    return psnr(y_gt, y_out, shave), ssim(y_gt, y_out)


def test_random_pairs_match_reference(fx):
    names = sorted({k.rsplit("/", 1)[0] for k in fx.files if k.startswith("rand/")})
    assert len(names) == 5
    for n in names:
        shave = int(n.rsplit("_s", 1)[1])
        p, s = _score(fx[n + "/gt"], fx[n + "/out"], shave)
        assert p == pytest.approx(fx[n + "/score"][0], abs=1e-5), n
        assert s == pytest.approx(fx[n + "/score"][1], abs=1e-12), n


def test_set5_scores_match_reference(fx):
    vals = []
    for k in sorted(k for k in fx.files if k.startswith("set5/")):
        stem = k.split("/")[1]
        out = np.array(Image.open(os.path.join(GOLDEN, "Set5", "ref_out", stem + "_LUT_ft_4bit.png")))
        gt = modcrop(np.array(Image.open(os.path.join(GOLDEN, "Set5", "HR", stem + ".png"))), 4)
        p, s = _score(gt, out, 4)
        assert p == pytest.approx(fx[k][0], abs=1e-5) and s == pytest.approx(fx[k][1], abs=1e-12), stem
        vals.append((p, s))
    m = np.mean(vals, axis=0)
    assert "{:.2f} {:.4f}".format(*m) == "30.61 0.8656"       # sr/4_test_lut.py:260 summary line


def test_scores_do_not_depend_on_concurrent_callers(fx):
    """The CLI scores finished images on several threads at once (eltr.run): the same five Set5 pairs scored by four threads,
    40 rounds, must give the single-threaded numbers every time (a BLAS matmul inside rgb2ycbcr did not)."""
    from concurrent.futures import ThreadPoolExecutor
    pairs = []
    for k in sorted(k for k in fx.files if k.startswith("set5/")):
        stem = k.split("/")[1]
        out = np.array(Image.open(os.path.join(GOLDEN, "Set5", "ref_out", stem + "_LUT_ft_4bit.png")))
        pairs.append((modcrop(np.array(Image.open(os.path.join(GOLDEN, "Set5", "HR", stem + ".png"))), 4), out))
    want = [_score(gt, out, 4) for gt, out in pairs]
    with ThreadPoolExecutor(4) as ex:
        for _ in range(40):
            assert list(ex.map(lambda p: _score(p[0], p[1], 4), pairs)) == want


# ---------------------------------------------------------------------------------------------------------------- full frames
def test_float32_and_float64_means_agree_within_the_psnr_bar_on_full_frames():
    """The reference takes np.mean of a float32 array of squared differences (pairwise float32 sums); mulut_eval_y adds the same
    float32 squares in float64 and rounds the mean to float32.  At 2 M pixels the two must still agree within the 1e-4 dB bar that
    test_gpu_eval.py holds the device to.  Measured: no difference at all on these four pairs (the two means round to the same float32; printed below)."""
    for name, (gt, out, shave) in big_pairs().items():
        d = rgb2ycbcr(out)[:, :, 0].astype(np.float32) - rgb2ycbcr(gt)[:, :, 0].astype(np.float32)
        d = d[shave:-shave, shave:-shave]
        sq = np.power(d, 2)
        assert sq.dtype == np.float32 and sq.size > 262144
        p32 = 20 * np.log10(255.0 / np.sqrt(np.mean(sq)))
        p64 = 20 * np.log10(255.0 / np.sqrt(np.float32(np.mean(sq, dtype=np.float64))))
        assert p32 == psnr(rgb2ycbcr(gt)[:, :, 0], rgb2ycbcr(out)[:, :, 0], shave)
        print(name, sq.size, "pixels: float32 mean %.9f dB, float64 mean %.9f dB, difference %.3g dB" % (p32, p64, abs(p32 - p64)))
        assert abs(p32 - p64) < 1e-5, name            # a tenth of the device test's bar
