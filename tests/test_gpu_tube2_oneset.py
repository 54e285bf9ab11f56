"""stage_tube2_kernel's one-set form (-m gpu): all four rotations of a channel in one accumulator set on the band staged in the
rotation-closed order (mulut_core.h tube4r_*; tests/test_tube2_oneset_cpu.py holds the placement and the arithmetic on the CPU).  The final stage is fed
directly with inputs whose pixels all lie on two adjacent MSB levels: every pass stays in the tube, so the fix-up list must stay EMPTY
-- the bytes compared with the oracle's are then the tube kernel's own, none repainted by the fix-up kernel.  Bar: bit-exact, 0 entries."""

import numpy as np
import pytest

import reach_cases as R
from oracle import c_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402

TABLES = ("random", "distinct", "all_max", "all_min")
LEVELS = (0, 7, 14)
# one full and one partial wave tile (16 x 4 sites) per row of tiles, H % 4 == 2; and a single full wave tile
SHAPES = ((2, 6, 19, 3), (1, 4, 16, 3))
ROWS = 17 ** 4


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def final_luts(kind):
    """Stage-2 tables of s, d, y, int8 [17^4][16]."""
    keysum = R.row_keys(4).sum(0)
    out = {}
    for i, m in enumerate("sdy"):
        if kind == "random":
            t = np.random.default_rng(100 + i).integers(-128, 128, (ROWS, 16))
        elif kind == "distinct":       # 7 q - 50 + (0 .. 6 by row and pattern): the 16 elements of a row all differ, so a misplaced field changes a byte
            t = 7 * np.arange(16)[None, :] - 50 + ((keysum + i) % 7)[:, None]
            assert all(len(set(row)) == 16 for row in t[:50].tolist()) and t.min() >= -128 and t.max() <= 127
        else:
            t = np.full((ROWS, 16), 127 if kind == "all_max" else -128)
        out["s2_" + m] = t.astype(np.int8)
    return out


def two_level(shape, level, seed):
    """Every pixel uniform in [16 level, 16 level + 31]: two adjacent MSB levels (edge replication adds no others)"""
    img = np.random.default_rng(seed).integers(16 * level, 16 * level + 32, shape).astype(np.uint8)
    assert set(np.unique(img >> 4).tolist()) == {level, level + 1}
    return img


def engine(modes, luts):
    e = MuLUTEngine(0).configure(2, modes, 4, 4).set_lut_dict(luts)
    # (last_detail_counters() reads the control block a context allocates with its first hybrid launch on planar input)
    e.stage(2, dev(np.full((3, 16, 64), 128, np.uint8)), layout=LAYOUT_CHW, out_layout=LAYOUT_HWC)
    e.set_tuning("final_stage_kernel", 5)       # the tube kernel on every tile: routing cannot send a tile elsewhere
    return e


def run_direct(e, modes, luts, tag):
    tables = [luts["s2_" + m] for m in modes]
    for shape in SHAPES:
        for level in LEVELS:
            img = two_level(shape, level, seed=level + shape[2])
            want = np.stack([c_oracle.stage(tables, modes, True, f, 4) for f in img])
            # HWC in, HWC out: the packed-RGB store; CHW in, CHW out: the planar store
            got_hwc = e.stage(2, dev(img), layout=LAYOUT_HWC).cpu().numpy()
            fix_hwc = e.last_detail_counters()["fix_pixels"]
            got_chw = e.stage(2, dev(img.transpose(0, 3, 1, 2)), layout=LAYOUT_CHW).cpu().numpy().transpose(0, 2, 3, 1)
            fix_chw = e.last_detail_counters()["fix_pixels"]
            print(tag, shape, "level", level, "fix entries", fix_hwc, fix_chw, "differing bytes", int((got_hwc != want).sum()), int((got_chw != want).sum()))
            assert fix_hwc == 0 and fix_chw == 0, (tag, shape, level, fix_hwc, fix_chw)
            assert np.array_equal(got_hwc, want), (tag, shape, level, "packed rgb")
            assert np.array_equal(got_chw, want), (tag, shape, level, "planar")


@pytest.mark.parametrize("modes", ["sdy", "sdys"])
@pytest.mark.parametrize("kind", TABLES)
def test_one_set_bytes_without_fixup(kind, modes):
    """sdys: M = 4, the s band is staged 2-fold -- with the all-+127 / all--128 tables the fields wrap on the way to K = 32512 / -32768."""
    luts = final_luts(kind)
    e = engine(modes, luts)
    assert e.kernel_name(2) == "stage_tube2_kernel<rgb,one-set>", e.kernel_name(2)
    assert "stage_tube2_kernel" in e.kernel_name(True)
    run_direct(e, modes, luts, (kind, modes))
    e.close()


def test_five_modes_keep_two_sets():
    """A numerator of five modes does not fit a signed 16-bit field: the list stays on two accumulator sets and the plain order."""
    luts = final_luts("random")
    e = engine("sdysd", luts)
    assert e.kernel_name(2) == "stage_tube2_kernel<rgb,two-set>", e.kernel_name(2)
    run_direct(e, "sdysd", luts, ("random", "sdysd"))
    e.close()


def test_cascade_with_flagged_samples(shipped_luts):
    """The whole cascade on photograph-like frames: samples leave the tube, so the new epilogue's bytes and the fix-up kernel's meet in
    one image; default routing (hybrid) and the tube kernel on every tile."""
    img = natural_frames(2, 38, 67, 3, 5)
    want = np.stack([c_oracle.pipeline(shipped_luts, 2, "sdy", 4, f) for f in img])
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(shipped_luts)
    assert e.kernel_name(2) == "stage_tube2_kernel<rgb,one-set>"
    for sel in (0, 5):
        e.set_tuning("final_stage_kernel", sel)
        got = e.pipeline(dev(img)).cpu().numpy()
        fix = e.last_detail_counters()["fix_pixels"]
        print("cascade final_stage_kernel", sel, "fix entries", fix, "differing bytes", int((got != want).sum()))
        assert np.array_equal(got, want), sel
        if sel == 5:
            assert fix > 0
    e.close()
