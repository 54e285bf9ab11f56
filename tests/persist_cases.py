"""Shared cases and reach measures of tests/test_persist_cpu.py and tests/test_gpu_persist.py (TEST ONLY; NumPy, the synthetic
frames and oracle/ alone -- nothing of the library under test).

A persistent kernel walks more work items than it has workgroups, and a fixed-grid list consumer strides over more entries than it
has threads; what either carries from one item to the next (a counter, an LDS flag, a list cursor, a clamp, a lane mask of a partial
tile) shows only on launches beyond the first pass.  The frames here are thin and tall: 67 pixels are two tile columns, the second
3 pixels wide (W % 64, W % 16 and W % 4 all nonzero), so a few thousand rows pass every limit at the cost of a small image.  Rows
alternate between photograph-like bands and uniform noise, with a period that is no multiple of 64 and not 16: tiles of 16 rows are
mostly of one kind, tiles of 64 rows mix, and one workgroup meets both kinds of work in turn.

The limits are those of a device with CUS compute units (the MI355X); the tile sizes and grid sizes restate the launchers."""
import functools
import os

import numpy as np

import flat_cases as F
import reach_cases as R
from mulut_amd.synth import natural_frames
from oracle import c_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CUS = 256
VERDICT_TILE = (64, 16)         # (width, height) of a tile of the x4 final stage: the tile statistic's verdicts, the tube kernels' work items
SITE_TILE = (64, 64)            # of the 1-byte-row and x2 / x3 tube kernels and of the window kernel's tile list
# consumer -> (what it walks, how much one pass of its grid covers)
LIMITS = {
    "tube": ("verdict_tiles", CUS),                 # stage_tube_kernel, stage_tube2_kernel: min(tiles, CUs) persistent workgroups
    "detail_plan": ("verdict_tiles", 1024),         # one block of 1024 threads
    "detail_retile": ("verdict_tiles", 8 * CUS),
    "detail_fill": ("verdict_tiles", 16 * CUS),
    "fix2": ("entries", 8 * CUS * 16),              # stage_up_fix2_kernel: 8 CUs blocks of 16 groups, grid stride
    "site_tiles": ("site_tiles", CUS),              # stage_u1w_kernel's list form and the 64 x 64 tube kernels: min(tiles, CUs) persistent
    "site_fix": ("entries", 4 * CUS * 256),         # stage_u1_fix_kernel, stage_up_fix_site_kernel<2>, <3>: 4 CUs blocks of 256 threads
}
# stage_slab_kernel (CUs workgroups over work items) is not here: its items are cut on the device, up to 4,096 samples each and about
# one per workgroup below that, so only a launch with more than CUs x 4,096 samples on the slabs passes its first round.  The two
# direct cases do; tests/test_gpu_persist.py asserts it there on the device's own item counter.
ONE_ROUND_MORE = ("detail_fill",)       # count > limit and count % limit != 0 is enough there: two full rounds would double the reference's cost

W = 67
PERIOD, NATURAL_ROWS = 80, 24           # rows [0, 24) of every 80 photograph-like, [24, 80) noise; each image starts at another phase
CALM_EVERY = 9                          # three periods of every nine have no noise band: 264 photograph-like rows, room for whole 64-row tiles
TABLE_KINDS = ("random", "checker")     # seeded random final tables, and 127 / -128 side by side: an unfixed sample reads the wrong sign


def case(n, h, c, stages, scale, modes, consumers, direct=False):
    """direct: the frames are the input of the final stage itself (the stages before it do not run)."""
    return {"n": n, "h": h, "w": W, "c": c, "stages": stages, "scale": scale, "modes": modes, "consumers": consumers, "direct": direct}


X4 = ("tube", "fix2")
CASES = {
    # 1. the x4 final stage fed directly
    "x4_final_c1": case(1, 33130, 1, 2, 4, "sdy", X4 + ("detail_plan", "detail_retile", "detail_fill"), direct=True),
    "x4_final_c3": case(1, 16650, 3, 2, 4, "sdy", X4 + ("detail_plan",), direct=True),
    # 2. two-stage x4 cascades, two images
    "x4_c1": case(2, 2090, 1, 2, 4, "sdy", X4),
    "x4_c2": case(2, 2090, 2, 2, 4, "sdy", X4),
    "x4_c3": case(2, 2090, 3, 2, 4, "sdy", X4),
    # 3. x4 lists off the sdy fast path
    "x4_sd_c1": case(2, 2090, 1, 2, 4, "sd", ("tube", "fix2")),
    "x4_sd_c2": case(2, 2090, 2, 2, 4, "sd", ("tube", "fix2")),
    "x4_sd_c3": case(2, 2090, 3, 2, 4, "sd", ("tube", "fix2")),
    "x4_sdysd_c1": case(2, 2090, 1, 2, 4, "sdysd", ("tube", "fix2")),
    "x4_sdysd_c2": case(2, 2090, 2, 2, 4, "sdysd", ("tube", "fix2")),
    "x4_sdysd_c3": case(2, 2090, 3, 2, 4, "sdysd", ("tube", "fix2")),
    # 4. x2 / x3 final stages
    "x2_c1": case(2, 8270, 1, 2, 2, "sdy", ("site_tiles", "site_fix")),
    "x2_c3": case(2, 8270, 3, 2, 2, "sdy", ("site_tiles", "site_fix")),
    "x3_c1": case(2, 8270, 1, 2, 3, "sdy", ("site_tiles", "site_fix")),
    "x3_c3": case(2, 8270, 3, 2, 3, "sdy", ("site_tiles", "site_fix")),
    "x2_sdysd_c3": case(2, 8270, 3, 2, 2, "sdysd", ("site_tiles", "site_fix")),
    # 5. deeper cascades: every stage with 1-byte rows passes the limits
    "x1_3stage": case(2, 8270, 2, 3, 1, "sdy", ("site_tiles", "site_fix")),
    "x2_4stage": case(2, 8270, 2, 4, 2, "sdy", ("site_tiles", "site_fix")),
}


# ---------------------------------------------------------------------------------------------
# content
# ---------------------------------------------------------------------------------------------
def ridges(h, w, k):
    """bool [h][w]: the steep two-pixel ridges of flat_cases.ridged, sparser -- diagonals a few hundred rows apart, so whole tiles
    stay without one --, one on the last column (it and its reach of two lie inside the partial tile column) on every fourth block of 48 rows, the one
    along the bottom edge on every column."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx + 3 * yy + k) % 787) < 2) | (((3 * xx - yy + k) % 1013) < 2) | ((xx == w - 1) & ((yy // 48) % 4 == 0))
            | (np.abs(yy - (h - 2)) < 1))


@functools.lru_cache(maxsize=None)
def frames(n, h, w, c, seed=0):
    """uint8 [n][h][w][c]: bands of natural_frames with ridges three MSB steps high, alternating with bands of uniform noise;
    three noise bands of every CALM_EVERY are left out (a tile of 64 rows mixes both kinds everywhere else: the stretches give the 64 x 64
    walkers tiles without a dirty sample too)."""
    img = natural_frames(n, h, w, c, seed=seed + 40).astype(np.int32)
    rng = np.random.default_rng([seed, n, h, w, c])
    noise = rng.integers(0, 256, (n, h, w, c))
    for f in range(n):
        rows = np.arange(h) + 24 * f
        calm = np.isin((rows // PERIOD) % CALM_EVERY, (3, 4, 5))
        # (the stretches without their pixel noise, which a cascade of first-stage tables sharpens stage by stage into dirty samples)
        img[f, calm] = np.rint(img[f, calm].mean(1, keepdims=True))
        for ch in range(c):
            img[f, :, :, ch] += 48 * ridges(h, w, 37 + 6 * ch + 11 * f)
        natural = ((rows % PERIOD) < NATURAL_ROWS) | calm
        img[f, ~natural] = noise[f, ~natural]
    out = np.clip(img, 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def case_frames(name):
    """The frames of a case; cases of one shape share them (and with them the non-final stages' outputs below)."""
    k = CASES[name]
    return frames(k["n"], k["h"], k["w"], k["c"], seed=k["h"] + k["c"])


# ---------------------------------------------------------------------------------------------
# tables and references
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shipped_first_stage(mode):
    """The first-stage table the reference ships for this pattern: 1-byte rows, valid at any scale.  Random tables in a non-final
    stage turn every frame into noise; these keep the photograph-like bands smooth for the stages behind them."""
    return np.load(os.path.join(GOLDEN, "luts", "LUT_ft_x4_4bit_int8_s1_%s.npy" % mode)).reshape(-1, 1)


@functools.lru_cache(maxsize=None)
def final_table(kind, mode, scale):
    if kind == "checker":
        return R.checker(4, scale * scale)
    return np.random.default_rng([ord(mode), scale]).integers(-128, 128, (17 ** 4, scale * scale), dtype=np.int8)


def luts(name, kind):
    """lut_dict of the case's cascade: shipped first-stage tables in every non-final stage, tables of `kind` in the final one."""
    k = CASES[name]
    out = {}
    for s in range(1, k["stages"] + 1):
        for m in set(k["modes"]):
            out["s%d_%s" % (s, m)] = final_table(kind, m, k["scale"]) if s == k["stages"] else shipped_first_stage(m)
    return out


@functools.lru_cache(maxsize=None)
def _stage_input(n, h, w, c, seed, modes, stage):
    if stage == 1:
        return frames(n, h, w, c, seed)
    tabs = [shipped_first_stage(m) for m in modes]
    x = np.stack([c_oracle.stage(tabs, modes, False, f, 1) for f in _stage_input(n, h, w, c, seed, modes, stage - 1)])
    x.setflags(write=False)
    return x


def stage_inputs(name):
    """The input of every stage, [stage - 1] -> uint8 [n][h][w][c], by the oracle: the frames, then the output of each non-final
    stage (shipped tables: they do not depend on the kind of the final tables, nor on the scale).  A direct case has the frames
    in every place."""
    k = CASES[name]
    return [_stage_input(k["n"], k["h"], k["w"], k["c"], k["h"] + k["c"], k["modes"], 1 if k["direct"] else s) for s in range(1, k["stages"] + 1)]


@functools.lru_cache(maxsize=4)
def reference(name, kind):
    """The oracle's bytes of the whole cascade, uint8 [n][h scale][w scale][c]."""
    k = CASES[name]
    tabs = [final_table(kind, m, k["scale"]) for m in k["modes"]]
    out = np.stack([c_oracle.stage(tabs, k["modes"], True, f, k["scale"]) for f in stage_inputs(name)[-1]])
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------
# reach measures
# ---------------------------------------------------------------------------------------------
def tile_count(n, rows, w, tile):
    return n * -(-w // tile[0]) * -(-rows // tile[1])


def tile_index(n, y, x, rows, w, tile):
    """Raster index of the tile that holds site (y, x) of image n: image-major, then tile row, then tile column."""
    return (n * -(-rows // tile[1]) + y // tile[1]) * -(-w // tile[0]) + x // tile[0]


@functools.lru_cache(maxsize=None)
def _dirty(n, h, w, c, seed, modes, stage):
    d = np.stack([F.dirty_mask(f) for f in _stage_input(n, h, w, c, seed, modes, stage)])
    d.setflags(write=False)
    return d


def dirty(name, stage):
    """flat_cases.dirty_mask of every image of the input of `stage`, bool [n][h][w][c]."""
    k = CASES[name]
    return _dirty(k["n"], k["h"], k["w"], k["c"], k["h"] + k["c"], k["modes"], 1 if k["direct"] else stage)


def tile_dirty_share(d, tile):
    """Per tile in raster order, (dirty samples, samples) of bool d [n][h][w][c]; a tile cut by the frame counts what lies inside."""
    n, h, w, c = d.shape
    tw, th = tile
    ty, tx = -(-h // th), -(-w // tw)
    cnt = np.zeros((n, ty * th, tx * tw), np.int64)
    cnt[:, :h, :w] = d.sum(3)
    one = np.zeros((ty * th, tx * tw), np.int64)
    one[:h, :w] = c
    dirty_per = cnt.reshape(n, ty, th, tx, tw).sum((2, 4)).reshape(-1)
    size_per = np.broadcast_to(one.reshape(ty, th, tx, tw).sum((1, 3)), (n, ty, tx)).reshape(-1)
    return dirty_per, size_per


def kinds_beyond(d, tile, limit, consumer=None):
    """(tiles without a dirty sample, tiles with more than half of their samples dirty) among the tiles of raster index >= limit;
    with `consumer`, among the tiles that consumer reaches in round 1 or later of its walk (walk_round: the persistent walkers stride
    over 8 ranges of the raster, so a tile of raster index >= limit can still be some workgroup's first)."""
    dirty_per, size_per = tile_dirty_share(d, tile)
    later = np.arange(len(dirty_per)) >= limit if consumer is None else walk_round(np.arange(len(dirty_per)), len(dirty_per), consumer) >= 1
    return int((dirty_per[later] == 0).sum()), int((2 * dirty_per[later] > size_per[later]).sum())


def reach(name, stage):
    """What the launch of `stage` of the case reaches, from its input alone: the tile counts and the reference's dirty samples."""
    k = CASES[name]
    return {"verdict_tiles": tile_count(k["n"], k["h"], k["w"], VERDICT_TILE), "site_tiles": tile_count(k["n"], k["h"], k["w"], SITE_TILE),
            "entries": int(dirty(name, stage).sum())}


def tile_of(consumer):
    return SITE_TILE if LIMITS[consumer][0] == "site_tiles" else VERDICT_TILE


def stages_of(name, consumer):
    """The stages of the case that run the consumer: the x4 consumers and the x2 / x3 site fix-up sit in the final stage, the
    1-byte-row ones in every stage with 1-byte rows."""
    k = CASES[name]
    return [s for s in range(1, k["stages"] + 1) if s == k["stages"] or consumer in ("site_tiles", "site_fix")]


def walk_round(idx, ntiles, consumer):
    """The round of the consumer's walk in which it reaches tile `idx` of `ntiles`.  The fixed grids stride over the raster: index //
    first-pass size.  The persistent tile walkers (CUs workgroups, a multiple of 8) cut the raster into 8 ranges of ceil(ntiles / 8)
    tiles, one per XCD, and CUs / 8 workgroups stride over each: (index % range) // (CUs / 8)."""
    limit = LIMITS[consumer][1]
    if consumer in ("tube", "site_tiles"):
        per = -(-ntiles // 8)
        return (idx % per) // (limit // 8)
    return idx // limit


def describe_difference(got, want, name, consumer, scale=None, row0=0):
    """Text for a failed comparison: how many bytes differ, the first few as (n, y, x, c) of the output, and which rounds of the
    consumer's walk over the tiles they fall in: 'rounds [1, 2]' reads as 'not the first pass'.  row0: got and want begin at this
    output row of the frame (a strip; y and the rounds are the whole frame's)."""
    k = CASES[name]
    s = k["scale"] if scale is None else scale
    if LIMITS[consumer][0] == "entries":
        consumer = "tube"
    tile = tile_of(consumer)
    at = np.argwhere(np.asarray(got) != np.asarray(want))
    at[:, 1] += row0
    idx = tile_index(at[:, 0], at[:, 1] // s, at[:, 2] // s, k["h"], k["w"], tile)
    rounds = np.unique(walk_round(idx, tile_count(k["n"], k["h"], k["w"], tile), consumer))
    text = "%s: %d bytes differ, first (n, y, x, c) %s; their %d x %d tiles lie in rounds %s of the walk (first pass: %d tiles)" % (
        name, len(at), [tuple(int(v) for v in a) for a in at[:4]], tile[0], tile[1], rounds.tolist()[:12], LIMITS[consumer][1])
    # A list consumer's rounds are rounds of list positions, which the bytes do not show (the order of a list is the order the tube
    # kernels' waves appended in).  What they show: a sample the fix-up pass never reached is one of the reference's dirty samples, and
    # no more of them can be missing than the list holds beyond one pass of the grid.
    d = dirty(name, k["stages"] if s == k["scale"] else 1)
    samples = np.unique(np.stack([at[:, 0], at[:, 1] // s, at[:, 2] // s, at[:, 3]], 1), axis=0)
    if len(samples) and (samples.max(0) < np.array(d.shape)).all():
        hit = d[samples[:, 0], samples[:, 1], samples[:, 2], samples[:, 3]]
        fix = LIMITS["fix2" if k["scale"] == 4 and s == 4 else "site_fix"][1]
        text += "; %d samples differ, %d of them dirty in the reference, which has %d dirty samples (one pass of the fix-up grid: %d)" % (
            len(samples), int(hit.sum()), int(d.sum()), fix)
    return text
