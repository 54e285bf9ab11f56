"""stage_up_fix2_kernel against the C oracle (-m gpu), cases from tests/fix2_cases.py (tests/test_fix2_cpu.py runs the kernel's
arithmetic for one sample on the CPU).  With the tube kernel on every tile and noise input the whole output is the fix-up kernel's
product.  Every call writes into a poisoned output, and the length of the work list (last_detail_counters()["fix_pixels"]) is held
to what the case means to produce.  Bar: bit-exact, counts as stated per test."""
import numpy as np
import pytest

import fix2_cases as X
from oracle import c_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402

LAYOUTS = (LAYOUT_HWC, LAYOUT_CHW)


def dev(x_nhwc, layout):
    x = x_nhwc if layout == LAYOUT_HWC else x_nhwc.transpose(0, 3, 1, 2)
    return torch.from_numpy(np.array(x, order="C", copy=True)).cuda()


def host(t, layout):
    a = t.cpu().numpy()
    return a if layout == LAYOUT_HWC else a.transpose(0, 2, 3, 1)


def poisoned(n, h, w, c, layout):
    return torch.full((n, h, w, c) if layout == LAYOUT_HWC else (n, c, h, w), X.POISON, dtype=torch.uint8, device="cuda")


def engine(modes, kind):
    """A two-stage x4 context of the list.  last_detail_counters() reads the control block of the detailed-tile path, which a context
    allocates with its first hybrid x4 launch on planar input: one such launch first."""
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(X.luts("sdy", "random"))
    e.stage(2, torch.full((3, 16, 64), 128, dtype=torch.uint8, device="cuda"), layout=LAYOUT_CHW, out_layout=LAYOUT_HWC)
    lut_dict = X.luts(modes, kind)
    e.configure(2, modes, 4, 4).set_lut_dict(lut_dict)
    return e, lut_dict


def final_stage(e, x, layout, out_layout):
    n, h, w, c = x.shape
    out = poisoned(n, 4 * h, 4 * w, c, out_layout)
    e.stage(2, dev(x, layout), layout=layout, out_layout=out_layout, out=out)
    return host(out, out_layout), e.last_detail_counters()["fix_pixels"]


def reference(lut_dict, modes, x):
    return np.stack([c_oracle.stage(X.final_tables(lut_dict, modes), modes, True, f, 4) for f in x])


def n_dirty(x, modes):
    return int(sum(X.dirty_mask(f, modes).sum() for f in x))


@pytest.mark.parametrize("modes,kind", [(m, k) for m, ks in X.LISTS.items() for k in ks])
def test_every_sample_through_the_fix_up(modes, kind):
    """Noise frames of 2 x 21 x 37, the tube kernel on every tile: (nearly) every sample is on the list, one, two and three channels,
    HWC and planar on either side.  sdys with the extreme tables holds the 16-bit fields at their bound; sdysd takes the any-list
    body.  The list is exactly the reference's dirty samples."""
    e, lut_dict = engine(modes, kind)
    e.set_tuning("final_stage_kernel", 5)
    for c in (1, 2, 3):
        x = X.noise(X.N, X.H, X.W, c, seed=c)
        want, dirty = reference(lut_dict, modes, x), n_dirty(x, modes)
        assert dirty >= 0.99 * x.size, (dirty, x.size)
        for layout in LAYOUTS:
            for out_layout in LAYOUTS:
                got, fix = final_stage(e, x, layout, out_layout)
                print(modes, kind, "C", c, "layouts", layout, out_layout, "fix entries", fix, "reference dirty samples", dirty, "of", x.size,
                      "differing bytes", int((got != want).sum()))
                assert fix == dirty, (c, layout, out_layout, fix, dirty)
                assert np.array_equal(got, want), (c, layout, out_layout)
    e.close()


@pytest.mark.parametrize("modes", ["sdy", "sdys"])
def test_strip_edges(modes):
    """The cascade in strips (0, 5), (5, 6), (6, 21): entries on the first and on the last row of a strip, their neighbours clamped
    to the rows the strip holds (or to the frame), in columns 0 and W - 1 too.  Each strip's list is the reference's dirty samples
    over that strip's rows of the first stage's output."""
    e, lut_dict = engine(modes, "random")
    x = X.noise(X.N, X.H, X.W, 3, seed=11)
    mid = np.stack([c_oracle.stage(X.first_tables(lut_dict, modes), modes, False, f, 1) for f in x])
    want = reference(lut_dict, modes, mid)
    dirty = np.stack([X.dirty_mask(f, modes) for f in mid])
    for layout in LAYOUTS:
        for y0, y1 in X.STRIPS:
            # the workspace keeps the first stage's output from call to call: the inverted frames go through it first
            e.set_tuning("final_stage_kernel", 1)
            e.pipeline(dev(255 - x, layout), layout=layout)
            e.set_tuning("final_stage_kernel", 5)
            r0, r1 = max(0, y0 - e.halo), min(X.H, y1 + e.halo)
            out = poisoned(X.N, 4 * (y1 - y0), 4 * X.W, 3, layout)
            e.pipeline_rows(dev(x[:, r0:r1], layout), r0, y0, y1, X.H, layout=layout, out=out)
            got, fix, ref = host(out, layout), e.last_detail_counters()["fix_pixels"], int(dirty[:, y0:y1].sum())
            print(modes, "strip", (y0, y1), "layout", layout, "fix entries", fix, "reference", ref, "of", dirty[:, y0:y1].size,
                  "differing bytes", int((got != want[:, 4 * y0:4 * y1]).sum()))
            assert fix == ref and ref >= 0.9 * dirty[:, y0:y1].size, (y0, y1, fix, ref)
            assert np.array_equal(got, want[:, 4 * y0:4 * y1]), (layout, y0, y1)
    e.close()


def test_entries_that_name_every_channel():
    """Default routing on a 40 x 131 frame, left half a smooth ramp, right half noise: the detailed tiles go to the slab path, which
    lists its border columns -- the frame's last six (a stage input fed by the caller is not padded), all 40 rows -- as entries for
    all three channels."""
    e, lut_dict = engine("sdy", "random")
    e.set_tuning("final_stage_kernel", 0)
    x = X.ramp_and_noise()
    want = reference(lut_dict, "sdy", x)
    for layout in LAYOUTS:
        got, fix = final_stage(e, x, layout, LAYOUT_HWC)
        d = e.last_detail_counters()
        print("layout", layout, "slab items", d["items"], "slab samples", sum(d["samples_per_anchor"]), "fix entries", fix,
              "differing bytes", int((got != want).sum()))
        assert np.array_equal(got, want), layout
        if layout == LAYOUT_CHW:        # (the hybrid's detailed-tile path takes planar input)
            assert d["items"] > 0 and sum(d["samples_per_anchor"]) > 0, d
            assert fix >= 6 * 40, fix
    e.close()


def test_short_and_empty_lists():
    """A 16 x 64 ramp with one 48-level step: the samples within two columns of the step are dirty, a few dozen entries for 2,048
    groups.  A constant frame: no entry at all -- the tube kernel overwrites the whole poisoned output, the fix-up leaves it alone."""
    e, lut_dict = engine("sdy", "random")
    e.set_tuning("final_stage_kernel", 5)
    x = X.step_edge(c=1)
    want, dirty = reference(lut_dict, "sdy", x), n_dirty(x, "sdy")
    assert 16 <= dirty <= 100, dirty
    for layout in LAYOUTS:
        got, fix = final_stage(e, x, layout, layout)
        print("step edge, layout", layout, "fix entries", fix, "reference", dirty, "differing bytes", int((got != want).sum()))
        assert fix == dirty and np.array_equal(got, want), (layout, fix, dirty)
    x = X.constant()
    want = reference(lut_dict, "sdy", x)
    assert n_dirty(x, "sdy") == 0
    for layout in LAYOUTS:
        got, fix = final_stage(e, x, layout, layout)
        print("constant, layout", layout, "fix entries", fix, "differing bytes", int((got != want).sum()))
        assert fix == 0 and np.array_equal(got, want), (layout, fix)
    e.close()


def test_more_entries_than_the_grid_has_groups():
    """8 x 64 x 256 noise frames: more listed samples than 8 workgroups x 16 groups per compute unit, so every group walks the list
    past its first entry (its sums cleared and read again, its pointers rebuilt)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x = X.noise(*X.MANY, seed=5)
    dirty = n_dirty(x, "sdy")
    if dirty <= cus * X.GROUPS_PER_CU:
        pytest.skip("%d compute units: the list of %d entries does not pass the grid's %d groups" % (cus, dirty, cus * X.GROUPS_PER_CU))
    e, lut_dict = engine("sdy", "random")
    e.set_tuning("final_stage_kernel", 5)
    want = reference(lut_dict, "sdy", x)
    for layout in LAYOUTS:
        got, fix = final_stage(e, x, layout, LAYOUT_HWC)
        print("layout", layout, "fix entries", fix, "reference", dirty, "groups", cus * X.GROUPS_PER_CU, "differing bytes", int((got != want).sum()))
        assert fix == dirty and np.array_equal(got, want), (layout, fix, dirty)
    e.close()
