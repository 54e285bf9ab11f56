"""The stage launcher at the index widths of its device work lists (-m gpu): 28 bits of byte offset on the anchor-slab path of x4
final stages, 30-bit pixel ids on the x4 fix-up list, 32-bit site ids on the 1-byte-row and x2 / x3 tube kernels (include/mulut.h,
"Batch size"), planes of 2^31 bytes or more and outputs beyond 2^32 bytes.

Section A needs no large buffer: mulut_pipeline_rows takes the height of the logical image apart from the band it is handed, and
the ids, the widths and the routes come from that height.  A strip at the bottom of a VIRTUAL frame a million rows tall runs with ids
next to 2^32 (2^30) on a few hundred kilobytes; its oracle is c_oracle.pipeline on the band (the strip and its halo) cropped to the
strip: the bottom of the band is the image's true border, its top is interior and the crop drops the halo rows the band's own top
border reaches.  Section B allocates what cannot be had otherwise.  Everything is bit-exact; no expectation comes from the library
except where a test says that it ALSO compares two of its routes with each other."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import c_oracle
from test_core_math_cpu import emul, run_emul  # noqa: F401  (the host emulator fixture and driver)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine, synthetic_lut  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402
from test_gpu_wide_patterns import emul_pipeline  # noqa: E402  (the cascade on the host emulator, for lists with e, h, o)

GiB = 1 << 30
W = 1024
# 32-bit site ids (1-byte rows, x2 / x3), C = 3:
H_SITES_BELOW = 1398016     # C * H * W = 4,294,705,152 <  2^32: one image stays on the tube route, two do not fit one launch
H_SITES_ABOVE = 1398144     # C * H * W = 4,295,098,368 >= 2^32: the window kernel (1-byte rows) / the gather kernel (x2, x3)
# 30-bit pixel ids (x4), C = 3:
H_PIXELS_BELOW = 1048512    # H * W = 1,073,676,288 < 2^30, and the first stage's sites C * H * W = 3,221,028,864 < 2^32
H_PIXELS_AT = 1048576       # H * W = 2^30: one image beyond the width
H_PIXELS_HALF = 524288      # H * W = 2^29: two images fit a first-stage launch (2 * 3 * 2^29 < 2^32 <= 3 * 3 * 2^29), one a final-stage launch
assert 3 * H_SITES_BELOW * W < 2 ** 32 <= 3 * H_SITES_ABOVE * W and 2 * 3 * H_SITES_BELOW * W >= 2 ** 32
assert H_PIXELS_BELOW * W < 2 ** 30 == H_PIXELS_AT * W and 3 * H_PIXELS_BELOW * W < 2 ** 32 <= 2 * 3 * H_PIXELS_BELOW * W
assert 2 * 3 * H_PIXELS_HALF * W < 2 ** 32 <= 3 * 3 * H_PIXELS_HALF * W and H_PIXELS_HALF * W < 2 ** 30 <= 2 * H_PIXELS_HALF * W
STRIP = 96
# channel 1's site ids ((C n + c) H + y) W + x cross 2^31 at y = 699,136: (H_SITES_BELOW + 699,136) * 1024 = 2^31
MIDDLE = (699100, 699200)
assert (H_SITES_BELOW + 699136) * W == 2 ** 31 and MIDDLE[0] < 699136 < MIDDLE[1]


@pytest.fixture(autouse=True)
def peak_device_memory(request):
    """Prints each test's peak of torch-allocated device memory; section A (test_a*) stays under 1 GiB."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("\n[peak device memory] %s: %.1f MiB" % (request.node.name, peak / 2 ** 20))
    torch.cuda.empty_cache()
    if request.node.name.startswith("test_a"):
        assert peak < GiB, peak


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@functools.lru_cache(maxsize=None)
def make_luts_cached(stages, modes, scale, interval=4):
    """Seeded random tables for the final stage (every wrong row shows).  The first stage of an s / d / y cascade at interval 4 gets
    the shipped first-stage tables instead: what a random table writes is noise everywhere, and then no tile of the final stage is
    smooth -- its tube kernel and fix-up list would run on nothing."""
    luts = {"s%d_%s" % (s + 1, m): synthetic_lut(17 + 31 * s + ord(m), scale * scale if s + 1 == stages else 1, interval)
            for s in range(stages) for m in set(modes)}
    if interval == 4 and stages == 2 and set(modes) <= set("sdy"):
        for m in set(modes):
            luts["s1_" + m] = np.load(os.path.join(GOLDEN, "luts", "LUT_ft_x4_4bit_int8_s1_%s.npy" % m)).reshape(-1, 1)
    return luts


def engine(stages, modes, scale, interval=4):
    return MuLUTEngine(0).configure(stages, modes, scale, interval).set_lut_dict(make_luts_cached(stages, modes, scale, interval))


@functools.lru_cache(maxsize=None)
def split_content(n, rows, w, c, seed=0):
    """Split content [n][rows][w][c]: the left half photograph-like, the right half uniform noise on every row of every image."""
    img = np.empty((n, rows, w, c), np.uint8)
    img[:, :, : w // 2] = natural_frames(n, rows, w // 2, c, seed=seed)
    img[:, :, w // 2:] = np.random.default_rng(seed + 1).integers(0, 256, (n, rows, w - w // 2, c), dtype=np.uint8)
    img.setflags(write=False)
    return img


def leaves_the_tube(rows_hwc):
    """The band criterion at interval 4, restated: a pass leaves the tube when the four MSBs (v >> 4) of its samples span more than
    one step.  True when some site of these rows has such a pass (the 2 x 2 pattern s at rotation 0 is enough)."""
    m = rows_hwc.astype(np.int32) >> 4
    four = np.stack([m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]])
    return bool(((four.max(0) - four.min(0)) > 1).any())


def assert_lists_reach_the_end(band, r0, y1):
    """On the input alone: within the last 16 rows of the strip, in the last image of the batch, some site has a pass outside the
    tube -- the highest ids of the launch are on the work lists."""
    assert leaves_the_tube(band[-1][y1 - 16 - r0:y1 - r0])


def strip_rows(e, h_full, y0, y1):
    halo = e.halo
    return max(0, y0 - halo), min(h_full, y1 + halo)


@functools.lru_cache(maxsize=None)
def oracle_strip(stages, modes, scale, n, c, rows, crop0, crop1, seed=0):
    """c_oracle.pipeline on each image of split_content(n, rows, W, c), cropped to LR rows [crop0, crop1) of the band."""
    luts = make_luts_cached(stages, modes, scale)
    band = split_content(n, rows, W, c, seed)
    return np.stack([c_oracle.pipeline(luts, stages, modes, scale, band[k])[crop0 * scale:crop1 * scale] for k in range(n)])


def run_strip(e, band, r0, y0, y1, h_full, layout=LAYOUT_HWC):
    """mulut_pipeline_rows on a band [n][rows][W][c] holding LR rows [r0, r0 + rows) of h_full-row images -> [n][rows'][W'][c]"""
    if layout == LAYOUT_HWC:
        return e.pipeline_rows(dev(band), r0, y0, y1, h_full, layout=layout).cpu().numpy()
    out = e.pipeline_rows(dev(band.transpose(0, 3, 1, 2)), r0, y0, y1, h_full, layout=layout)
    return out.cpu().numpy().transpose(0, 2, 3, 1)


def strip_case(e, stages, modes, scale, h_full, y0, y1, n=1, c=3):
    """(band, r0, expected) of the strip [y0, y1) of n h_full-row images of split content"""
    r0, r1 = strip_rows(e, h_full, y0, y1)
    band = split_content(n, r1 - r0, W, c)
    assert_lists_reach_the_end(band, r0, y1)
    return band, r0, oracle_strip(stages, modes, scale, n, c, r1 - r0, y0 - r0, y1 - r0)


def counters(e):
    d = e.last_detail_counters()
    print("[work counters] slab samples %d, fix-up entries %d" % (sum(d["samples_per_anchor"]), d["fix_pixels"]))
    return sum(d["samples_per_anchor"]), d["fix_pixels"]


# ---------------------------------------------------------------------------------------------
# A. ids and widths through tall virtual frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["top", "middle", "bottom"])
def test_a1_site_ids_up_to_2_32_on_the_tube_route(where):
    """1-byte-row stages of one image with C H W just under 2^32: the strip at the bottom has site ids within 2^18 of 2^32, the middle
    one channel-1 ids crossing 2^31, the top one is the control.  Both layouts equal the oracle, and (in addition) the window kernel
    on every tile (first_stage_kernel 2: no lists)."""
    h = H_SITES_BELOW
    y0, y1 = {"top": (0, STRIP), "middle": MIDDLE, "bottom": (h - STRIP, h)}[where]
    e = engine(2, "sdy", 1)
    band, r0, want = strip_case(e, 2, "sdy", 1, h, y0, y1)
    if where == "bottom":                           # ids of channel 2, ((2 H + y) W + x: from 2^32 - 360,448 to 2^32 - 2^18 - 1
        assert 2 ** 32 - 3 * h * W == 2 ** 18 and 2 ** 32 - (2 * h + y0) * W < 2 ** 19
    for layout in (LAYOUT_HWC, LAYOUT_CHW):
        got = run_strip(e, band, r0, y0, y1, h, layout)
        assert np.array_equal(got, want), (where, layout)
        e.set_tuning("first_stage_kernel", 2)
        assert np.array_equal(run_strip(e, band, r0, y0, y1, h, layout), got), (where, layout, "window kernel")
        e.set_tuning("first_stage_kernel", 0)
    e.set_tuning("first_stage_kernel", 3)           # the tube kernel on every tile: every site out of the band on the list
    assert np.array_equal(run_strip(e, band, r0, y0, y1, h), want), (where, "tube kernel on every tile")
    e.close()


def test_a1_two_images_run_as_two_sub_launches():
    """N = 2 of the bottom strip: one image takes (nearly) all 32 bits, so every stage runs as two sub-launches of one image."""
    h = H_SITES_BELOW
    e = engine(2, "sdy", 1)
    band, r0, want = strip_case(e, 2, "sdy", 1, h, h - STRIP, h, n=2)
    for layout in (LAYOUT_HWC, LAYOUT_CHW):
        got = run_strip(e, band, r0, h - STRIP, h, h, layout)
        assert np.array_equal(got, want), layout
    e.set_tuning("first_stage_kernel", 2)
    assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h), want)
    e.close()


@pytest.mark.parametrize("n", [1, 2])
def test_a2_window_kernel_at_2_32_sites(n):
    """C H W >= 2^32: the 1-byte-row stages fall back to the window kernel (32-bit site ids cannot name the sites).  The band is the
    bottom strip's again, so the oracle's bytes are the same as below the width."""
    h = H_SITES_ABOVE
    e = engine(2, "sdy", 1)
    band, r0, want = strip_case(e, 2, "sdy", 1, h, h - STRIP, h, n=n)
    for layout in (LAYOUT_HWC, LAYOUT_CHW):
        assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h, layout), want), layout
    for first in (3, 2):
        e.set_tuning("first_stage_kernel", first)
        assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h), want), first
    e.close()


@pytest.mark.parametrize("scale,stages", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_a3_x2_x3_final_stages_at_2_32_sites(scale, stages):
    """x2 / x3 final stages: the tube-band family with its site fix-up below 2^32 site ids, the gather kernel at or above; default
    tuning (routed), the tube kernel on every tile (5) and the gather kernel (1) each equal the oracle.  Below the width also the
    strip where channel 1's ids cross 2^31 and a batch of two (two sub-launches)."""
    e = engine(stages, "sdy", scale)
    for h in (H_SITES_BELOW, H_SITES_ABOVE):
        band, r0, want = strip_case(e, stages, "sdy", scale, h, h - STRIP, h)
        for sel in (0, 5, 1):
            e.set_tuning("final_stage_kernel", sel)
            assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h), want), (h, sel)
        e.set_tuning("final_stage_kernel", 0)
        assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h, LAYOUT_CHW), want), (h, "planar")
        band2, r02, want2 = strip_case(e, stages, "sdy", scale, h, h - STRIP, h, n=2)
        assert np.array_equal(run_strip(e, band2, r02, h - STRIP, h, h), want2), (h, "N = 2")
    h = H_SITES_BELOW
    band, r0, want = strip_case(e, stages, "sdy", scale, h, *MIDDLE)
    for sel in (0, 5):
        e.set_tuning("final_stage_kernel", sel)
        assert np.array_equal(run_strip(e, band, r0, MIDDLE[0], MIDDLE[1], h), want), ("middle", sel)
    e.close()


def test_a4_pixel_ids_up_to_2_30_one_image():
    """x4 cascade of one image with H W just under 2^30 (pixel ids of the fix-up list within 2^17 of 2^30, first-stage site ids
    up to 3 * 2^30): the hybrid, the tube kernels on every tile, the gather kernel on the detailed tiles -- all equal the oracle, and
    the work counters say which path ran."""
    h = H_PIXELS_BELOW
    e = engine(2, "sdy", 4)
    band, r0, want = strip_case(e, 2, "sdy", 4, h, h - STRIP, h)
    assert 2 ** 30 - (h - STRIP) * W < 2 ** 18
    for layout in (LAYOUT_HWC, LAYOUT_CHW):
        assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h, layout), want), layout
        slab, fix = counters(e)
        assert slab > 0 and fix > 0, (layout, slab, fix)                  # hybrid: detailed tiles on the anchor slabs
    for pipelined in (1, 0):
        e.set_tuning("final_stage_kernel", 5).set_tuning("tube_pipelined", pipelined)
        assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h), want), ("tube", pipelined)
        slab, fix = counters(e)
        assert slab == 0 and fix > 0, (pipelined, slab, fix)              # every tile on the tube kernel: no slab work, a long fix-up list
    e.set_tuning("final_stage_kernel", 0).set_tuning("tube_pipelined", 1).set_tuning("detail_kernel", 1)
    assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h), want), "detail_kernel 1"
    slab, fix = counters(e)
    assert slab == 0 and fix > 0, (slab, fix)                             # documented: the gather kernel takes the detailed tiles
    e.set_tuning("detail_kernel", 0).set_tuning("stat_from_first_stage", 0)
    assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h), want), "stat_from_first_stage 0"
    e.close()


@pytest.mark.parametrize("n,h", [(2, H_PIXELS_BELOW), (5, H_PIXELS_HALF)])
def test_a4_batches_split_in_both_stages(n, h):
    """N = 2 just under 2^30 pixels: both stages run one image per sub-launch.  N = 5 at H W = 2^29: the first stage fits two images
    (sub-launches 2 + 2 + 1), the final stage one (1 x 5) -- the final stage's sub-launches do not line up with the first stage's, whose
    tile marks a split first stage must not hand on.  The last image ends on noise: its samples are on the last sub-launch's lists."""
    e = engine(2, "sdy", 4)
    band, r0, want = strip_case(e, 2, "sdy", 4, h, h - STRIP, h, n=n)
    for layout in (LAYOUT_HWC, LAYOUT_CHW):
        assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h, layout), want), layout
        slab, fix = counters(e)
        assert slab > 0 and fix > 0, (layout, slab, fix)
    for key, val in (("stat_from_first_stage", 0), ("first_stage_kernel", 3), ("final_stage_kernel", 5)):
        e.set_tuning(key, val)
        assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h), want), (key, val)
    e.close()


def test_a5_one_x4_image_at_2_30_pixels_takes_the_gather_kernel():
    """One x4 image with H W = 2^30: 30-bit pixel ids cannot name its pixels, so the final stage runs on the gather kernel (as the
    1-byte-row and x2 / x3 families fall back at 2^32) and gives the oracle's bytes; a fresh context's work counters stay empty -- no
    hybrid or tube launch ran -- where the same band one row block lower (test_a4) fills them."""
    h = H_PIXELS_AT
    for n in (1, 2):
        e = engine(2, "sdy", 4)
        band, r0, want = strip_case(e, 2, "sdy", 4, h, h - STRIP, h, n=n)
        for layout in (LAYOUT_HWC, LAYOUT_CHW):
            assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h, layout), want), (n, layout)
        assert counters(e) == (0, 0)
        e.set_tuning("final_stage_kernel", 5)
        assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h), want), (n, "final_stage_kernel 5")
        assert counters(e) == (0, 0)
        e.close()


@pytest.mark.parametrize("scale,h", [(1, H_SITES_BELOW), (4, H_PIXELS_BELOW)])
@pytest.mark.parametrize("modes,c", [("sdysd", 3), ("sdy", 1), ("sdy", 5)])
def test_a6_mode_lists_and_channel_counts_at_the_widths(scale, h, modes, c):
    """Five modes, one channel and five channels (two groups, each a view with the caller's strides) at the shapes of A1 and A4, one
    image and two (sub-launches), both layouts."""
    e = engine(2, modes, scale)
    if scale == 4 and len(modes) > 3:       # (the counters are read from the slab path's control words: allocate them on a list it takes)
        e.configure(2, "sdy", 4)
        e.pipeline(dev(split_content(1, 100, W, 3)))
        assert counters(e)[0] > 0
        e.configure(2, modes, 4)
    for n in (1, 2):
        band, r0, want = strip_case(e, 2, modes, scale, h, h - STRIP, h, n=n, c=c)
        for layout in (LAYOUT_HWC, LAYOUT_CHW):
            assert np.array_equal(run_strip(e, band, r0, h - STRIP, h, h, layout), want), (n, layout)
            if scale == 4:
                slab, fix = counters(e)
                assert fix > 0 and (slab > 0) == (len(modes) <= 3), (n, layout, slab, fix)      # the anchor slabs take three modes at most
    e.close()


def test_sizes_beyond_the_launch_fields_are_refused():
    """Sizes that the int fields of a launch cannot hold return MULUT_EUNSUPPORTED from every entry point before any launch (the
    buffers here are a few bytes: a call that went on would fault)."""
    e = engine(2, "sdy", 4)
    x = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    y = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    lib, hnd, EUNSUPPORTED = e._lib, e._h, -5
    absurd = [(1, 4, 1 << 29, 3),           # a packed output row of W * 4 * 3 bytes
              (1, 1 << 30, 4, 3),           # H * 4 output rows
              (1 << 20, 1 << 20, 1 << 20, 1),   # 2^32 tiles of 32 x 8 sites
              (1, 4, (1 << 31) - 1, 1)]
    for n, h, w, c in absurd:
        for layout in (LAYOUT_HWC, LAYOUT_CHW):
            assert lib.mulut_pipeline(hnd, x.data_ptr(), y.data_ptr(), n, h, w, c, layout, None) == EUNSUPPORTED, (n, h, w, c)
            assert lib.mulut_pipeline_rows(hnd, x.data_ptr(), 0, h, y.data_ptr(), 0, h, n, h, w, c, layout, None) == EUNSUPPORTED, (n, h, w, c)
            for stage in (1, 2):
                assert lib.mulut_stage(hnd, stage, x.data_ptr(), layout, y.data_ptr(), layout, n, h, w, c, None) == EUNSUPPORTED, (n, h, w, c)
        assert lib.mulut_reserve(hnd, n, h, w, c) == EUNSUPPORTED, (n, h, w, c)
    torch.cuda.synchronize()
    assert "unsupported" in lib.mulut_strerror(EUNSUPPORTED).decode()
    img = split_content(1, 8, 16, 3)[0]                                  # and the context still works
    assert np.array_equal(e.pipeline(dev(img)).cpu().numpy(), c_oracle.pipeline(make_luts_cached(2, "sdy", 4), 2, "sdy", 4, img))
    e.close()


# ---------------------------------------------------------------------------------------------
# B. what needs a large buffer
# ---------------------------------------------------------------------------------------------
def need_device_memory(need):
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %d bytes of free device memory, the device reports %d" % (need, free))


def big_split_planar(c, h, w, seed):
    """Split content [c][h][w] built on the device: the left half a 1024 x 2050 photograph-like tile repeated, the right half uniform
    noise (torch's generator; the oracle reads the same bytes back)."""
    tile = torch.from_numpy(natural_frames(1, 1024, 2050, c, seed=seed)[0].transpose(2, 0, 1).copy()).cuda()
    x = torch.empty((c, h, w), dtype=torch.uint8, device="cuda")
    half = w // 2
    assert h % 1024 == 0 and half % 2050 == 0
    x[:, :, :half] = tile.repeat(1, h // 1024, half // 2050)
    g = torch.Generator(device="cuda").manual_seed(seed)
    for y in range(0, h, 4096):         # (in row blocks: the generator's scratch stays small)
        x[:, y:y + 4096, half:] = torch.randint(0, 256, (c, min(4096, h - y), w - half), dtype=torch.uint8, device="cuda", generator=g)
    return x


def equal_permuted(hwc, chw, block=2048):
    """hwc [H][W][C] == chw [C][H][W], compared on the device in row blocks"""
    return all(torch.equal(hwc[y:y + block].permute(2, 0, 1), chw[:, y:y + block]) for y in range(0, hwc.shape[0], block))


def check_windows_planar(x, out, luts, stages, modes, scale, halo, corners):
    """96 x 96 LR windows of a planar frame x [C][H][W] recomputed by the oracle with the cascade's halo, against out [C][H s][W s]"""
    _, h, w = x.shape
    for (y, xx) in corners:
        y0, y1, x0, x1 = max(0, y - halo), min(h, y + 96 + halo), max(0, xx - halo), min(w, xx + 96 + halo)
        ref = c_oracle.pipeline(luts, stages, modes, scale, x[:, y0:y1, x0:x1].permute(1, 2, 0).contiguous().cpu().numpy())
        ref = ref[(y - y0) * scale:(y - y0 + 96) * scale, (xx - x0) * scale:(xx - x0 + 96) * scale]
        got = out[:, y * scale:(y + 96) * scale, xx * scale:(xx + 96) * scale].permute(1, 2, 0).contiguous().cpu().numpy()
        assert np.array_equal(got, ref), (y, xx)


B1_NEED = 14 * GiB      # 4.0 GiB per output (two held), 0.25 GiB per input (two), 0.5 GiB of workspace, 1.5 GiB of work lists, strips


def test_b1_output_plane_of_2_31_bytes_planar():
    """2-stage sdy x4 on one planar 2-channel LR frame of 8192 x 16400: each output plane has 32768 * 65600 = 2,149,580,800 bytes
    (>= 2^31: plane 1 is out of reach of a 32-bit channel stride), and the stage input's 268,697,600 bytes pass 2^28, the header's
    "single image beyond 2^28 bytes": its detailed tiles take the gather kernel and the slab counters read zero.  Against the oracle
    on windows (corners, centre, across byte offset 2^31 of plane 0; every window in both planes), against the packed layout (channel
    stride 1) and against eight strips (small planes), whole outputs compared on the device."""
    need_device_memory(B1_NEED)
    c, h, w, s = 2, 8192, 16400, 4
    assert (h * s) * (w * s) == 2149580800 >= 2 ** 31 and c * h * w == 268697600 >= 2 ** 28
    luts = make_luts_cached(2, "sdy", 4)
    e = engine(2, "sdy", 4)
    small = split_content(1, 100, W, 2)
    e.pipeline(dev(small))
    assert counters(e)[0] > 0                               # (the slab path runs on a small frame: the counters are live)
    x = big_split_planar(c, h, w, seed=3)
    assert leaves_the_tube(x[1, h - 16:, :].cpu().numpy())  # plane 1 ends on noise: the last ids are on the lists
    out = e.pipeline(x[None], layout=LAYOUT_CHW)[0]
    slab, fix = counters(e)
    assert slab == 0 and fix > 0, (slab, fix)
    assert tuple(out.shape) == (c, h * s, w * s)
    # byte offset 2^31 of plane 0 is HR row 32736, column 2048: LR (8184, 512), inside the window at (8096, 464)
    assert 32736 * (w * s) + 2048 == 2 ** 31
    corners = [(0, 0), (0, w - 96), (h - 96, 0), (h - 96, w - 96), (h // 2 - 48, w // 2 - 48), (h - 96, 464)]
    check_windows_planar(x, out, luts, 2, "sdy", s, e.halo, corners)
    hwc = e.pipeline(x.permute(1, 2, 0).contiguous())
    assert equal_permuted(hwc, out)
    del hwc
    halo = e.halo
    for k in range(8):
        y0, y1 = k * h // 8, (k + 1) * h // 8
        r0, r1 = max(0, y0 - halo), min(h, y1 + halo)
        part = e.pipeline_rows(x[None, :, r0:r1].contiguous(), r0, y0, y1, h, layout=LAYOUT_CHW)[0]
        assert torch.equal(part, out[:, y0 * s:y1 * s]), k
        del part
    e.close()


B2_NEED = 20 * GiB      # 4.0 GiB each: planar input, planar output, packed input, packed output; strips of 0.5 + 0.5 GiB


def test_b2_input_plane_of_2_31_bytes():
    """1-stage s at scale 1 on one planar 2-channel frame of 32768 x 65600: input and output planes of 2,149,580,800 bytes, and
    C H W >= 2^32 (the window kernel).  The same three checks as B1."""
    need_device_memory(B2_NEED)
    c, h, w = 2, 32768, 65600
    assert h * w == 2149580800 >= 2 ** 31
    luts = make_luts_cached(1, "s", 1)
    e = engine(1, "s", 1)
    x = big_split_planar(c, h, w, seed=5)
    out = e.pipeline(x[None], layout=LAYOUT_CHW)[0]
    assert 32736 * w + 2048 == 2 ** 31                      # byte offset 2^31 of plane 0: row 32736, column 2048
    corners = [(0, 0), (0, w - 96), (h - 96, 0), (h - 96, w - 96), (h // 2 - 48, w // 2 - 48), (h - 96, 2000)]
    check_windows_planar(x, out, luts, 1, "s", 1, e.halo, corners)
    xh = x.permute(1, 2, 0).contiguous()
    hwc = e.pipeline(xh)
    del xh
    assert equal_permuted(hwc, out)
    del hwc
    halo = e.halo
    for k in range(8):
        y0, y1 = k * h // 8, (k + 1) * h // 8
        r0, r1 = max(0, y0 - halo), min(h, y1 + halo)
        part = e.pipeline_rows(x[None, :, r0:r1].contiguous(), r0, y0, y1, h, layout=LAYOUT_CHW)[0]
        assert torch.equal(part, out[:, y0:y1]), k
        del part
    e.close()


B3_NEED = 8 * GiB       # 4.1 GiB of output, 0.26 GiB of input, 0.5 GiB of workspace, the two reference frames
B3_CASES = [(4, "sdyeho", "stage_wide_up_kernel"),                       # the wide kernels
            (6, "sdy", "stage_interval_kernel<6,4,lds>"),                # tables in LDS (at x4 an sdy list fits 96 KiB at interval 6 only)
            (5, "sdy", "stage_interval_kernel<5,4,global>")]             # rows gathered from global memory


@pytest.mark.parametrize("interval,modes,kernel", B3_CASES)
def test_b3_outputs_beyond_2_32_bytes(emul, interval, modes, kernel):  # noqa: F811
    """44 frames of 1080 x 1920 x 3 at x4 = 4,379,443,200 output bytes (> 2^32) through the kernels that have no work lists and so
    never split: the wide kernels and stage_interval_kernel on both of its routes.  Two distinct split-content frames repeated; every
    image equals its frame-by-frame result (two calls of the library, in addition to:) the two frames equal the emulator (wide list)
    or the oracle (intervals 5, 6) on windows with the halo.  Both layouts."""
    need_device_memory(B3_NEED)
    n, h, w, s = 44, 1080, 1920, 4
    assert n * h * s * w * s * 3 == 4379443200 > 2 ** 32
    luts = make_luts_cached(2, modes, s, interval)
    e = engine(2, modes, s, interval)
    assert kernel in e.kernel_name(True), e.kernel_name(True)
    base = split_content(2, h, w, 3, seed=7)
    assert leaves_the_tube(base[1][h - 16:])
    halo = e.halo
    for layout in (LAYOUT_HWC, LAYOUT_CHW):
        b = dev(base if layout == LAYOUT_HWC else base.transpose(0, 3, 1, 2))
        ref = e.pipeline(b, layout=layout)
        host = ref.cpu().numpy() if layout == LAYOUT_HWC else ref.cpu().numpy().transpose(0, 2, 3, 1)
        for k in range(2):
            for (y, xx) in ((0, 0), (h - 96, w - 96), (h // 2 - 48, w // 2 - 48)):
                y0, y1, x0, x1 = max(0, y - halo), min(h, y + 96 + halo), max(0, xx - halo), min(w, xx + 96 + halo)
                win = np.ascontiguousarray(base[k][y0:y1, x0:x1])
                want = (emul_pipeline(emul, luts, 2, modes, s, win) if interval == 4
                        else c_oracle.pipeline(luts, 2, modes, s, win, interval=interval))
                want = want[(y - y0) * s:(y - y0 + 96) * s, (xx - x0) * s:(xx - x0 + 96) * s]
                assert np.array_equal(host[k][y * s:(y + 96) * s, xx * s:(xx + 96) * s], want), (layout, k, y, xx)
        out = e.pipeline(b.repeat(n // 2, 1, 1, 1).contiguous(), layout=layout)
        assert out.numel() == 4379443200
        for k in range(n):
            assert torch.equal(out[k], ref[k % 2]), (layout, k)
        del out, ref, b
    e.close()
