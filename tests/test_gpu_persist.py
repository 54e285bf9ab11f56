"""Persistent kernels and fixed-grid list consumers past their first pass (-m gpu): thin, tall, band-mixed frames from
tests/persist_cases.py (tests/test_persist_cpu.py asserts on the reference alone what they reach) through every route that walks
tiles with min(tiles, CUs) workgroups or strides over a work list with a fixed grid.  State kept from one tile or entry to the next
-- a counter, an LDS flag, a list cursor, a clamp, a partial tile's lane mask -- gives wrong bytes only here.
Bar: np.array_equal with the oracle, no tolerance; the work counters confirm on the device that the lists were as long as claimed.
A failure names the round of the walk (tile index // first-pass size) the differing bytes fall in."""
import numpy as np
import pytest

import persist_cases as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402

GiB = 1 << 30
DEFAULTS = {"final_stage_kernel": 0, "first_stage_kernel": 0, "tube_pipelined": 1, "detail_kernel": 0, "stat_from_first_stage": 1,
            "hybrid_oob_per_1024": 128, "first_stage_detail_per_1024": 24, "final_stage_detail_per_1024": 8}
LAYOUTS = (LAYOUT_HWC, LAYOUT_CHW)


@pytest.fixture(autouse=True, scope="module")
def device_is_no_larger_than_the_cases_assume():
    """The first-pass sizes of persist_cases are those of 256 compute units: a larger device would pass these tests vacuously."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus <= P.CUS, "the cases pass the limits of %d compute units, this device has %d" % (P.CUS, cus)


@pytest.fixture(autouse=True)
def peak_device_memory(request):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("\n[peak device memory] %s: %.1f MiB" % (request.node.name, peak / 2 ** 20))
    torch.cuda.empty_cache()
    assert peak < 2 * GiB, peak


def dev(x_nhwc, layout):
    x = x_nhwc if layout == LAYOUT_HWC else x_nhwc.transpose(0, 3, 1, 2)
    return torch.from_numpy(np.array(x, order="C", copy=True)).cuda()


def host(t, layout):
    a = t.cpu().numpy()
    return a if layout == LAYOUT_HWC else a.transpose(0, 2, 3, 1)


def engine(name, kind):
    """A context of the case's cascade.  last_detail_counters() reads the control block of the detailed-tile path, which a context
    allocates with its first hybrid x4 launch on planar input: one such launch first, whatever the case's own configuration."""
    k = P.CASES[name]
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(P.luts("x4_c3", "random"))
    e.stage(2, torch.full((3, 16, 64), 128, dtype=torch.uint8, device="cuda"), layout=LAYOUT_CHW, out_layout=LAYOUT_HWC)
    e.configure(k["stages"], k["modes"], k["scale"], 4).set_lut_dict(P.luts(name, kind))
    tune(e)
    return e


def tune(e, **keys):
    for key, value in dict(DEFAULTS, **keys).items():
        e.set_tuning(key, value)


def same(got, want, name, consumer, tag, scale=None, row0=0):
    print(name, tag, "differing bytes", int((got != want).sum()) if got.shape == want.shape else "shape")
    assert got.shape == want.shape, (name, tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        pytest.fail("%s -- %s" % (tag, P.describe_difference(got, want, name, consumer, scale, row0)), pytrace=False)


POISON = 0xA5
SCRUB = {"first_stage_kernel": 2, "final_stage_kernel": 1}      # the window kernel and the gather kernel on every tile: no list, no walker


def poisoned(n, h, w, c, layout):
    """An output buffer full of POISON.  Every call here writes into one: the allocator would otherwise hand a call the block the
    call before it has just freed, with that call's correct bytes still in it, and a tile left unwritten would compare equal."""
    return torch.full((n, h, w, c) if layout == LAYOUT_HWC else (n, c, h, w), POISON, dtype=torch.uint8, device="cuda")


def scrub(e, x, layout):
    """The same holds for the context's workspace, where the non-final stages' outputs stay from call to call: before a cascade runs
    under the tuning in question, the inverted frames go through it on the kernels without lists or persistent walkers."""
    if e.stages > 1:
        tune(e, **SCRUB)
        e.pipeline(dev(255 - x, layout), layout=layout)


def pipeline(e, keys, x, layout):
    """The cascade under the tuning `keys`, on a scrubbed workspace, into a poisoned output."""
    scrub(e, x, layout)
    tune(e, **keys)
    n, h, w, c = x.shape
    out = poisoned(n, h * e.scale, w * e.scale, c, layout)
    e.pipeline(dev(x, layout), layout=layout, out=out)
    return host(out, layout)


def strip(e, keys, x, y0, y1, layout):
    """Rows [y0, y1) of the cascade's output from the smallest band it reads, as pipeline()."""
    scrub(e, x, layout)
    tune(e, **keys)
    n, h, w, c = x.shape
    r0, r1 = max(0, y0 - e.halo), min(h, y1 + e.halo)
    out = poisoned(n, (y1 - y0) * e.scale, w * e.scale, c, layout)
    e.pipeline_rows(dev(x[:, r0:r1], layout), r0, y0, y1, h, layout=layout, out=out)
    return host(out, layout)


def stage(e, s, x, layout=LAYOUT_CHW, out_layout=LAYOUT_HWC):
    """One stage under the tuning that is set, into a poisoned output (a single stage does not touch the workspace)."""
    n, h, w, c = x.shape
    u = e.scale if s == e.stages else 1
    out = poisoned(n, h * u, w * u, c, out_layout)
    e.stage(s, dev(x, layout), layout=layout, out_layout=out_layout, out=out)
    return host(out, out_layout)


def fix_entries(e, name, s, tag):
    """The length of the fix-up list of the last launch, printed beside the reference's dirty samples of that stage's input."""
    fix = e.last_detail_counters()["fix_pixels"]
    print(name, tag, "stage", s, "fix-up entries", fix, "reference dirty samples", int(P.dirty(name, s).sum()))
    return fix


def hybrid_counters(e, name, tag, past_one_round):
    """The slab path ran; past_one_round: on more work items than stage_slab_kernel has workgroups (more than CUs x 4,096 samples)."""
    d = e.last_detail_counters()
    print(name, tag, "slab items", d["items"], "slab samples", sum(d["samples_per_anchor"]), "fix-up entries", d["fix_pixels"])
    assert d["items"] > (P.CUS if past_one_round else 0) and sum(d["samples_per_anchor"]) > 0, (name, tag, d)


# ---------------------------------------------------------------------------------------------
# 1. the x4 final stage fed directly, planar input
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.TABLE_KINDS)
@pytest.mark.parametrize("name", ["x4_final_c1", "x4_final_c3"])
def test_x4_final_stage_fed_directly(name, kind):
    """More than 4,096 verdict tiles on one channel (every kernel of the detailed-tile path takes a second round, the tube kernels
    a seventeenth), more than 2,048 on three; the hybrid at three thresholds, either tube kernel, either detail kernel, the tube
    kernels on every tile (tube2: the fix-up list is exactly the reference's dirty samples) and the gather kernel."""
    e = engine(name, kind)
    x, want = P.stage_inputs(name)[-1], P.reference(name, kind)
    n_dirty = int(P.dirty(name, 2).sum())
    for keys in ({}, {"hybrid_oob_per_1024": 0}, {"hybrid_oob_per_1024": 128}, {"hybrid_oob_per_1024": 1024}, {"tube_pipelined": 0},
                 {"detail_kernel": 1}, {"final_stage_kernel": 1}, {"final_stage_kernel": 5}, {"final_stage_kernel": 5, "tube_pipelined": 0}):
        tune(e, **keys)
        same(stage(e, 2, x), want, name, "tube", keys)
        if keys.get("final_stage_kernel") == 5:
            fix = fix_entries(e, name, 2, keys)
            if "tube_pipelined" not in keys:
                assert "stage_tube2_kernel" in e.kernel_name(True) and fix == n_dirty, (keys, fix, n_dirty)
            else:
                assert "stage_tube_kernel" in e.kernel_name(True) and fix > P.LIMITS["fix2"][1], (keys, fix)
        elif not keys or keys.get("hybrid_oob_per_1024") == 0:      # (threshold 0: every tile with a sample out of the band is detailed)
            hybrid_counters(e, name, keys, past_one_round=True)
    tune(e)
    same(stage(e, 2, x, LAYOUT_CHW, LAYOUT_CHW), want, name, "tube", "planar output")
    same(stage(e, 2, x, LAYOUT_HWC, LAYOUT_HWC), want, name, "tube", "HWC input")
    e.close()


# ---------------------------------------------------------------------------------------------
# 2. two-stage x4 cascades
# ---------------------------------------------------------------------------------------------
X4_TUNINGS = ({}, {"first_stage_kernel": 2}, {"first_stage_kernel": 3}, {"stat_from_first_stage": 0}, {"final_stage_kernel": 5})


@pytest.mark.parametrize("kind", P.TABLE_KINDS)
@pytest.mark.parametrize("name", ["x4_c1", "x4_c2", "x4_c3"])
def test_x4_cascade(name, kind):
    """Two different images, 524 verdict tiles: both layouts under the tunings that change which kernels walk them; the frame as
    two strips cut at a row that is no multiple of 16, each with the smallest band the cascade reads."""
    e = engine(name, kind)
    k = P.CASES[name]
    x, want = P.case_frames(name), P.reference(name, kind)
    for keys in X4_TUNINGS:
        for layout in LAYOUTS:
            same(pipeline(e, keys, x, layout), want, name, "tube", (keys, "layout %d" % layout))
    h, cut = k["h"], 1043
    assert cut % 16 and cut % 4
    for layout in LAYOUTS:
        for y0, y1 in ((0, cut), (cut, h)):
            same(strip(e, {}, x, y0, y1, layout), want[:, 4 * y0:4 * y1], name, "tube", ("strip", y0, y1, "layout %d" % layout), row0=4 * y0)
    tune(e)
    # the final stage alone on the oracle's first-stage output: what the lists held
    mid = P.stage_inputs(name)[1]
    same(stage(e, 2, mid), want, name, "tube", "final stage alone")
    hybrid_counters(e, name, "final stage alone", past_one_round=False)      # (under 2^20 samples: the slab kernel's items fit one round)
    tune(e, final_stage_kernel=5)
    same(stage(e, 2, mid), want, name, "tube", "final stage alone, tube kernel on every tile")
    fix, n_dirty = fix_entries(e, name, 2, "tube2 on every tile"), int(P.dirty(name, 2).sum())
    assert fix == n_dirty, (fix, n_dirty)
    e.close()


# ---------------------------------------------------------------------------------------------
# 3. x4 lists off the sdy fast path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.TABLE_KINDS)
@pytest.mark.parametrize("name", ["x4_sd_c1", "x4_sd_c2", "x4_sd_c3", "x4_sdysd_c1", "x4_sdysd_c2", "x4_sdysd_c3"])
def test_x4_other_lists(name, kind):
    """sd runs on stage_tube_kernel (tube2 takes lists that hold all of s, d, y), sdysd on tube2 with the per-rotation gather kernel
    on the detailed tiles.  With a tube kernel on every tile, tube2 leaves exactly the reference's dirty samples on the list also for
    five modes (a repeated pattern flags the same samples); stage_tube_kernel on sd flags fewer (no y passes): more than a first pass."""
    e = engine(name, kind)
    k = P.CASES[name]
    x, want = P.case_frames(name), P.reference(name, kind)
    tube = "stage_tube_kernel" if k["modes"] == "sd" else "stage_tube2_kernel"
    assert tube in e.kernel_name(True), e.kernel_name(True)
    if k["modes"] == "sdysd":
        assert "wide" in e.kernel_name(True), e.kernel_name(True)
    for keys in ({}, {"first_stage_kernel": 3}, {"final_stage_kernel": 5}):
        same(pipeline(e, keys, x, LAYOUT_HWC), want, name, "tube", keys)
    mid = P.stage_inputs(name)[1]
    tune(e, final_stage_kernel=5)
    same(stage(e, 2, mid), want, name, "tube", "final stage alone, tube kernel on every tile")
    fix, n_dirty = fix_entries(e, name, 2, tube + " on every tile"), int(P.dirty(name, 2).sum())
    assert fix > P.LIMITS["fix2"][1] and (fix == n_dirty or k["modes"] == "sd"), (fix, n_dirty)
    e.close()


# ---------------------------------------------------------------------------------------------
# 4. x2 / x3 final stages
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.TABLE_KINDS)
@pytest.mark.parametrize("name", ["x2_c1", "x2_c3", "x3_c1", "x3_c3", "x2_sdysd_c3"])
def test_x2_x3_final_stages(name, kind):
    """520 tiles of 64 x 64 in both stages and more than two passes of the site fix-up kernels' grid: routed at three thresholds,
    the tube kernel on every tile, the gather kernel; both layouts."""
    e = engine(name, kind)
    k = P.CASES[name]
    x, want = P.case_frames(name), P.reference(name, kind)
    for keys in ({}, {"final_stage_detail_per_1024": 0}, {"final_stage_detail_per_1024": 8}, {"final_stage_detail_per_1024": 1024},
                 {"final_stage_kernel": 5}, {"final_stage_kernel": 1}):
        for layout in LAYOUTS:
            same(pipeline(e, keys, x, layout), want, name, "site_tiles", (keys, "layout %d" % layout))
    tune(e, final_stage_kernel=5)
    mid = P.stage_inputs(name)[1]
    same(stage(e, 2, mid), want, name, "site_tiles", "final stage alone, tube kernel on every tile")
    assert fix_entries(e, name, 2, "stage_u1t_kernel<%d> on every tile" % k["scale"]) > P.LIMITS["site_fix"][1]
    e.close()


# ---------------------------------------------------------------------------------------------
# 5. deeper cascades
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.TABLE_KINDS)
@pytest.mark.parametrize("name", ["x1_3stage", "x2_4stage"])
def test_deeper_cascades(name, kind):
    """Every stage with 1-byte rows walks 520 tiles of 64 x 64 and fixes up more than two passes' worth of sites: the routed kernels
    at three thresholds, the window kernel and the tube kernel on every tile; then each non-final stage alone against the oracle's
    next input, with the tube kernel on every tile and the length of its list."""
    e = engine(name, kind)
    k = P.CASES[name]
    x, want = P.case_frames(name), P.reference(name, kind)
    for keys in ({}, {"first_stage_detail_per_1024": 0}, {"first_stage_detail_per_1024": 24}, {"first_stage_detail_per_1024": 1024},
                 {"first_stage_kernel": 2}, {"first_stage_kernel": 3}):
        for layout in (LAYOUTS if not keys else (LAYOUT_HWC,)):
            same(pipeline(e, keys, x, layout), want, name, "site_tiles", (keys, "layout %d" % layout))
    inputs = P.stage_inputs(name)
    for s in range(1, k["stages"]):
        for first in (0, 3):
            tune(e, first_stage_kernel=first)
            same(stage(e, s, inputs[s - 1]), inputs[s], name, "site_tiles", "stage %d alone, first_stage_kernel %d" % (s, first), scale=1)
        assert fix_entries(e, name, s, "stage_u1t_kernel on every tile") > P.LIMITS["site_fix"][1]
    e.close()
