"""stage_tube2_kernel's flat-tile skip and its per-wave fix-up count (-m gpu).  Crafted final-stage inputs from tests/flat_cases.py
(tests/test_flat_cpu.py asserts on the reference alone what they are) go straight to the final stage.  Every run is held to the oracle's
bytes; with the tube kernel on every tile the length of the fix-up list must also equal the reference's exact number of dirty samples
-- a tube test skipped where it was needed, or an entry lost on a partial tile, changes that number even where the bytes agree.
Bar: bit-exact, counts equal."""

import numpy as np
import pytest

import flat_cases as F
import reach_cases as R
from oracle import c_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402

CASES = F.small_cases()
TABLES = ("shipped", "checker")       # the shipped tables and an extreme kind: a sample left unflagged reads a band entry of the wrong sign


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.fixture(scope="module")
def engines(shipped_luts):
    out = {}
    for kind in TABLES:
        luts = shipped_luts if kind == "shipped" else R.cascade_luts(kind, 2, "sdy", 4, 4)
        e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(luts)
        e.set_tuning("tube_pipelined", 1)
        # last_detail_counters() reads the control block of the detailed-tile path, which a context allocates with its first hybrid
        # launch on planar input: one such launch before the tube kernel runs alone
        e.stage(2, dev(np.full((3, 16, 64), 128, np.uint8)), layout=LAYOUT_CHW, out_layout=LAYOUT_HWC)
        out[kind] = (e, luts)
    yield out
    for e, _ in out.values():
        e.close()


def final_tables(luts):
    return [luts["s2_%s" % m] for m in "sdy"]


def run_final(e, img, planar):
    """One frame (HWC) or a batch (NHWC) through the final stage: planar input takes the kernel's dword path (W % 4 == 0), HWC its byte path."""
    if planar:
        x = img.transpose(2, 0, 1) if img.ndim == 3 else img.transpose(0, 3, 1, 2)
        return e.stage(2, dev(x), layout=LAYOUT_CHW, out_layout=LAYOUT_HWC).cpu().numpy()
    return e.stage(2, dev(img), layout=LAYOUT_HWC).cpu().numpy()


def check(e, img, want, n_dirty, tag):
    assert img.shape[-2] % 4 == 0
    for planar in (True, False):
        for sel in (5, 0):
            e.set_tuning("final_stage_kernel", sel)
            if sel == 5:
                assert "stage_tube2_kernel" in e.kernel_name(True), e.kernel_name(True)
            got = run_final(e, img, planar)
            fix = e.last_detail_counters()["fix_pixels"]
            print(tag, "planar" if planar else "HWC", "final_stage_kernel", sel, "fix entries", fix, "reference dirty samples", n_dirty,
                  "differing bytes", int((got != want).sum()))
            assert np.array_equal(got, want), tag + (planar, sel)
            if sel == 5:
                assert fix == n_dirty, tag + (planar, fix, n_dirty)
    e.set_tuning("final_stage_kernel", 0)


@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_outlier_positions(engines, name, kind):
    e, luts = engines[kind]
    img = CASES[name][0]
    want = c_oracle.stage(final_tables(luts), "sdy", True, img, 4)
    check(e, img, want, int(F.dirty_mask(img).sum()), (name, kind))


@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("shape", F.PARTIAL_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_persistent_waves_on_partial_tiles(engines, shape, kind):
    """More work items than waves, edge tiles cut by the frame: a wave goes from a partial tile to a full one with entries in its buffer."""
    e, luts = engines[kind]
    img = F.ridged(*shape)
    want = np.stack([c_oracle.stage(final_tables(luts), "sdy", True, f, 4) for f in img])
    check(e, img, want, int(sum(F.dirty_mask(f).sum() for f in img)), (shape, kind))


def test_strips(engines, shipped_luts):
    """The cascade in two strips of 135 rows (the final stage's row clamps): bytes of the whole-frame oracle, and with the tube kernel on
    every tile the fix-up list of each strip is the reference's dirty count over that strip's rows of the first stage's output."""
    e, luts = engines["shipped"]
    n, h, w, half = 2, 270, 500, 135
    img = natural_frames(n, h, w, 3, 4)
    mid = [c_oracle.stage([luts["s1_%s" % m] for m in "sdy"], "sdy", False, f, 1) for f in img]
    want = np.stack([c_oracle.stage(final_tables(luts), "sdy", True, f, 4) for f in mid])
    dirty = np.stack([F.dirty_mask(f) for f in mid])
    for sel in (5, 0):
        e.set_tuning("final_stage_kernel", sel)
        halo = e.halo
        for y0, y1 in ((0, half), (half, h)):
            r0, r1 = max(y0 - halo, 0), min(y1 + halo, h)
            got = e.pipeline_rows(dev(img[:, r0:r1]), r0, y0, y1, h).cpu().numpy()
            fix = e.last_detail_counters()["fix_pixels"]
            print("strip", (y0, y1), "final_stage_kernel", sel, "fix entries", fix, "reference", int(dirty[:, y0:y1].sum()))
            assert np.array_equal(got, want[:, 4 * y0:4 * y1]), (sel, y0, y1)
            if sel == 5:
                assert fix == int(dirty[:, y0:y1].sum()), (y0, y1, fix)
    e.set_tuning("final_stage_kernel", 0)
