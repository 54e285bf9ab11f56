"""stage_up_fix2_kernel's entry-level skip against the C oracle (-m gpu), cases from tests/fix2_skip_cases.py (tests/test_fix2_skip_cpu.py
holds the argument and shows on the oracle alone that these frames carry a few hundred flagged samples of either kind and that a wrongly
skipped sample would change bytes).  The kernel leaves an entry alone when a tube kernel listed it and every pass of the sample has its
values within 32 levels; the entries of the slab path's border columns, which name every channel, it always computes.  Every call writes
into a poisoned output, so a sample nobody computed shows.  Bar: bit-exact; the list's length stays what the MSB rule gives
(fix2_cases.dirty_mask) -- the skip changes what the kernel does with an entry, not what is listed."""
import numpy as np
import pytest

import fix2_cases as X
import fix2_skip_cases as S
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


def engine(modes, lut_dict):
    """A two-stage x4 context of the list (last_detail_counters() reads the control block a context allocates with its first hybrid x4
    launch on planar input: one such launch first)."""
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(X.luts("sdy", "random"))
    e.stage(2, torch.full((3, 16, 64), 128, dtype=torch.uint8, device="cuda"), layout=LAYOUT_CHW, out_layout=LAYOUT_HWC)
    e.configure(2, modes, 4, 4).set_lut_dict(lut_dict)
    return e


def final_stage(e, x, layout, out_layout):
    n, h, w, c = x.shape
    out = poisoned(n, 4 * h, 4 * w, c, out_layout)
    e.stage(2, dev(x, layout), layout=layout, out_layout=out_layout, out=out)
    return host(out, out_layout), e.last_detail_counters()["fix_pixels"]


def reference(lut_dict, modes, x):
    return np.stack([c_oracle.stage(X.final_tables(lut_dict, modes), modes, True, f, 4) for f in x])


@pytest.mark.parametrize("modes,kind", [("sdy", "random")] + [("sdys", k) for k in X.LISTS["sdys"]] + [("sdysd", "random")])
def test_listed_samples_of_both_kinds(modes, kind):
    """The tube kernel on every tile, frames of 2 x 21 x 37, 40 x 131 and 2 x 21 x 40 (planar rows of whole dwords) with steep ramps, steps
    of exactly 32 and 33 levels, noise and a smooth band; one, two and three channels, HWC and planar on either side.  sdys with the extreme tables holds the recomputed samples'
    16-bit fields at their bound; sdysd takes the any-list body, which recomputes every entry."""
    lut_dict = X.luts(modes, kind)
    e = engine(modes, lut_dict)
    e.set_tuning("final_stage_kernel", 5)
    for shape in S.SHAPES:
        for c in (1, 2, 3):
            x = S.frames(*shape, c)
            want = reference(lut_dict, modes, x)
            dirty = int(sum(X.dirty_mask(f, modes).sum() for f in x))
            skip, keep = (sum(v) for v in zip(*[S.census(f, modes) for f in x]))
            assert skip >= 200 and keep >= 200 and skip + keep == dirty, (skip, keep, dirty)
            for layout in LAYOUTS:
                for out_layout in LAYOUTS:
                    got, fix = final_stage(e, x, layout, out_layout)
                    print(modes, kind, shape, "C", c, "layouts", layout, out_layout, "fix entries", fix, "MSB rule", dirty, "of them skippable", skip,
                          "differing bytes", int((got != want).sum()))
                    assert fix == dirty, (shape, c, layout, out_layout, fix, dirty)
                    assert np.array_equal(got, want), (shape, c, layout, out_layout)
    e.close()


def bordered(c):
    """40 x 131: noise in columns 5 .. 120 (the 64 x 16 tiles at x0 = 0 and x0 = 64 are detailed), a slow ramp in columns 0 .. 4 and
    121 .. 130: the slab path lists columns 0, 1 and 125 .. 127 of its tiles as entries that name every channel, and every pass of those
    samples is within 32 levels."""
    h, w = 40, 131
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.repeat((90 + (xx + yy) // 3)[..., None], c, axis=2) + 9 * np.arange(c)
    img[:, 5:121] = X.noise(1, h, 116, c, seed=21)[0]
    return img.astype(np.uint8)[None]


@pytest.mark.parametrize("c", [1, 2, 3])
def test_border_entries_of_the_slab_path_are_always_computed(c):
    """Default routing.  The border samples look skippable (no pass is far) but no tube kernel has computed them: skipped, they would
    keep the poison.  With fewer than three channels the entries still name every channel."""
    lut_dict = X.luts("sdy", "random")
    e = engine("sdy", lut_dict)
    e.set_tuning("final_stage_kernel", 0)
    x = bordered(c)
    want = reference(lut_dict, "sdy", x)
    border = [0, 1, 125, 126, 127]
    assert not S.far_mask(x[0], "sdy")[:, border].any()
    for layout in LAYOUTS:
        got, fix = final_stage(e, x, layout, LAYOUT_HWC)
        d = e.last_detail_counters()
        print("C", c, "layout", layout, "slab items", d["items"], "slab samples", sum(d["samples_per_anchor"]), "fix entries", fix,
              "differing bytes", int((got != want).sum()), "poison left", int((got == X.POISON).sum()), "expected by chance", int((want == X.POISON).sum()))
        assert np.array_equal(got, want), (c, layout)
        if layout == LAYOUT_CHW:        # (the hybrid's detailed-tile path takes planar input)
            assert d["items"] > 0 and sum(d["samples_per_anchor"]) > 0, d
            assert fix >= len(border) * 40, fix
    e.close()


@pytest.mark.parametrize("modes", ["sdy", "sdys"])
def test_strips(modes):
    """The cascade in strips (0, 5), (5, 6), (6, 21) behind a first stage that hands the frame through: the predicate sees neighbours
    clamped to the rows the strip holds.  Each strip's list is the MSB rule's over that strip's rows; over the strips both kinds of listed
    samples occur by the hundred."""
    lut_dict = dict(X.luts(modes, "random"))
    lut_dict.update(S.identity_first_tables(modes))
    e = engine(modes, lut_dict)
    x = S.frames(X.N, X.H, X.W, 3)
    mid = np.stack([c_oracle.stage(X.first_tables(lut_dict, modes), modes, False, f, 1) for f in x])
    assert np.abs(mid.astype(int) - x.astype(int)).max() <= 2          # (the top level of an int8 table clips)
    want = reference(lut_dict, modes, mid)
    skip, keep = (sum(v) for v in zip(*[S.census(f, modes, rows) for f in mid for rows in X.STRIPS]))
    assert skip >= 200 and keep >= 200, (skip, keep)
    for layout in LAYOUTS:
        for y0, y1 in X.STRIPS:
            # the workspace keeps the first stage's output from call to call: the inverted frames go through it first
            e.set_tuning("final_stage_kernel", 1)
            e.pipeline(dev(255 - x, layout), layout=layout)
            e.set_tuning("final_stage_kernel", 5)
            r0, r1 = max(0, y0 - e.halo), min(X.H, y1 + e.halo)
            out = poisoned(X.N, 4 * (y1 - y0), 4 * X.W, 3, layout)
            e.pipeline_rows(dev(x[:, r0:r1], layout), r0, y0, y1, X.H, layout=layout, out=out)
            got, fix = host(out, layout), e.last_detail_counters()["fix_pixels"]
            ref = int(sum(X.dirty_mask(f, modes)[y0:y1].sum() for f in mid))
            print(modes, "strip", (y0, y1), "layout", layout, "fix entries", fix, "MSB rule", ref, "differing bytes", int((got != want[:, 4 * y0:4 * y1]).sum()))
            assert fix == ref, (y0, y1, fix, ref)
            assert np.array_equal(got, want[:, 4 * y0:4 * y1]), (layout, y0, y1)
    e.close()
