"""Cases and harness of the fine-tune half of the C ABI (test infrastructure, shared by test_ft_abi_cpu.py and test_gpu_ft_abi.py;
nothing is imported from the code under test).

include/mulut.h promises for mulut_ft_quantize(_backward), the four families of mulut_ft*_stage_forward / _backward and
mulut_eval_y: stateless and stream-ordered, float alignment suffices, nothing outside a buffer is read or written, the backward
ADDS into grad_wq and grad_x.  The cases are the exact-integer cases of tests/ft_exact_cases.py and tests/ft_wide_cases.py (integer
tables, integer x, grad_out = avg * k: every output is the oracle's bytes in any summation order), picked so that every kernel
instance and its edges are reached -- reach_of() restates the launch rules in NumPy and test_ft_abi_cpu.py asserts the coverage.

  Arena     every pointer of a call is carved out of ONE allocation, each buffer between two slacks of its own of SLACK bytes, at
            a chosen byte offset past a 16-byte boundary.  Slack around outputs holds FILL bytes, around float inputs NaN, around
            the clamp mask of a backward all-ones: a store beside a buffer changes the arena, a load beside an input that is
            used shows in the result.
  prefill   seeded integers over q for grad_wq and grad_x: the backward must give prefill + reference, a second call
            prefill + 2 * reference, in every element; the exactness cap of the sum is asserted on the reference alone.
  clamp     interval-4 cases with a handful of pixels outside 0..255, infinite and NaN: which sites and pixels they can reach."""
import copy
import functools
import zlib

import numpy as np

import ft_exact_cases as fx
import ft_wide_cases as fw

CAP = fx.CAP
SLACK = 1024                     # bytes of slack before and after every buffer of an arena
FILL = 0xA5                      # slack around outputs
OFFSETS = (0, 4, 8, 12)          # byte offset of every float buffer past a 16-byte boundary; 0: the run the others are compared with
PREFILL = 64                     # prefilled numerators lie in -PREFILL .. PREFILL
LDS_BUDGET = 120 * 1024          # kFtIvLdsBudget of mulut_ft_interval.hip
GX_TILE = 1024                   # floats of a wave's input-gradient tile (kFtGxTile, kFtIvGxTile)


# ------------------------------------------------------------------------------------------------------------------ the case list
def _pick(cases, **want):
    hit = [c for c in cases if all(getattr(c, k) == v for k, v in want.items())]
    assert len(hit) == 1, (want, [c.name for c in hit])
    return hit[0]


def is_wide(case):
    return any(m in "eho" for m in case.modes)


def entries_of(case):
    """the entry-point families a case runs through: plain / mask (interval 4), interval (5, 6), wide (all)"""
    if is_wide(case):
        return ("wide",)
    return ("plain", "mask", "wide") if case.interval == 4 else ("interval", "wide")


def _cases():
    out = []
    for iv in (4, 5, 6):
        for u in (1, 2, 3, 4):       # ragged 4 x 4 blocks, two planes, tiles that straddle a plane boundary
            out.append(_pick(fx.CASES, interval=iv, u=u, last=1, modes="sdy", shape=(2, 1, 13, 10), content="noise"))
            out.append(_pick(fx.CASES, interval=iv, u=u, last=0, modes="sdy", shape=(1, 2, 9, 11), content="noise"))
        # the halo tile is larger than the image on every side
        out.append(_pick(fx.CASES, interval=iv, shape=(1, 1, 1, 1)))
        out.append(_pick(fx.CASES, interval=iv, shape=(1, 1, 1, 7)))
        out.append(_pick(fx.CASES, interval=iv, shape=(1, 1, 9, 1)))
        # the memory fallback of the input-gradient tile
        out.append(_pick(fx.CASES, interval=iv, u=1, shape=(1, 2, 3, 300)))
        out.append(_pick(fx.CASES, interval=iv, u=4, shape=(1, 2, 3, 300)))
        out.append(_pick(fx.CASES, interval=iv, u=2, shape=(1, 1, 4, 260)))
        # a 4 x 4 pattern in the list: the halo-3 instances, through the wide entry points
        out.append(_pick(fw.CASES, interval=iv, u=1, modes="sdyeho", shape=(1, 2, 9, 11)))
        out.append(fw.WideCase(iv, 4, 1, "sdyeho", (2, 1, 13, 10), "noise", reach=("inside",)))
    # persistent workgroups: several tiles per workgroup, flushes from many workgroups, rows outside the band -- one per family
    out.append(_pick(fx.CASES, interval=4, u=4, modes="sdy", shape=(16, 1, 48, 48), content="noise"))
    out.append(_pick(fx.CASES, interval=4, u=1, modes="sdy", shape=(16, 1, 48, 48), content="noise"))
    out.append(_pick(fx.CASES, interval=5, u=4, modes="sdy", shape=(16, 1, 48, 48), content="noise"))
    out.append(_pick(fx.CASES, interval=6, u=1, modes="sdy", shape=(16, 1, 48, 48), content="noise"))
    out.append(_pick(fw.CASES, interval=4, u=4, modes="eho", shape=(16, 1, 48, 48), content="noise"))
    assert len(set(c.name for c in out)) == len(out)
    return out


CASES = _cases()
LARGEST = 16 * 1 * 48 * 48


@functools.lru_cache(maxsize=None)
def _built(name):
    case = copy.copy(next(c for c in CASES + EXTRA if c.name == name)).build()
    ref = (fw.reference if is_wide(case) else fx.reference)(case)
    return case, ref


def built(case):
    """(a copy of the case with tables, x and gout in place, its integer reference): computed once per process and shared -- read only.
    A copy, because the objects of CASES are those of ft_exact_cases.CASES / ft_wide_cases.CASES, which the tests that own those lists
    build and release (`case.tables = case.x = case.gout = None`) per test: in one process with them the cache must not hold theirs."""
    return _built(case.name)


# ------------------------------------------------------------------------------------------------ the launch rules, restated
def rows_of(interval):
    return (2 ** (8 - interval) + 1) ** 4


def halo_of(case):
    return 3 if is_wide(case) else 2


def wave_tiles_fit(case):
    """per wave of 64 consecutive sites of the one-site-per-thread backward kernels (u < 4): does its input-gradient tile -- the
    stacked rows its sites lie in plus the halo on either side, each plane with halo rows and columns of its own -- fit GX_TILE
    floats?  (ft_stage_bwd / ft_interval_stage_bwd: when it does not, the adds go to memory)"""
    B, C, H, W = case.shape
    halo, nsite = halo_of(case), B * C * H * W
    pw = W + 2 * halo

    def padded_row(R):
        return R + 2 * halo * (R // H) + halo
    fits = []
    for w0 in range(0, nsite, 64):
        r0, r1 = w0 // W, min(w0 + 63, nsite - 1) // W
        t_rows = padded_row(r1) + halo - (padded_row(r0) - halo) + 1
        fits.append(t_rows * pw <= GX_TILE)
    return fits


def reach_of(case):
    """the kernel instances and forms one forward + one backward of the case launch, as names: a restatement of launch_ft
    (mulut_ft.hip) and launch_ftiv_fwd / launch_ftiv_bwd (mulut_ft_interval.hip) -- u, interval, halo, and whether the table image
    fits the LDS budget"""
    iv, u, halo = case.interval, case.u, halo_of(case)
    fam = "iv4" if iv == 4 else "iv56"
    out = set()
    if iv == 4:
        out.add("iv4:fwd<%d>" % u)
        out.add("iv4:bwd4<halo%d>" % halo if u == 4 else "iv4:bwd<%d,halo%d>" % (u, halo))
        if u in (1, 4):
            out.add("iv4:band")                        # the tube band in LDS (u = 1: per workgroup, u = 4: per workgroup and mode)
    else:
        image = rows_of(iv) * u * u * 4
        out.add("iv56:fwd<%d,%d,%s>" % (iv, u, "lds" if case.M * image <= LDS_BUDGET else "global"))
        res = image <= LDS_BUDGET
        if u == 4:
            out.add("iv56:bwd4<%d,%s,halo%d>" % (iv, "resident" if res else "band", halo))
        else:
            out.add("iv56:bwd<%d,%d,%s,halo%d>" % (iv, u, "resident" if res else "memory", halo))
    if u < 4:
        fits = wave_tiles_fit(case)
        out.add(fam + (":gx_tile" if all(fits) else ":gx_memory" if not any(fits) else ":gx_mixed"))
    return out


def required_reach():
    need = set()
    for u in (1, 2, 3, 4):
        need.add("iv4:fwd<%d>" % u)
        for iv in (5, 6):
            for M in (3,):
                need.add("iv56:fwd<%d,%d,%s>" % (iv, u, "lds" if M * rows_of(iv) * u * u * 4 <= LDS_BUDGET else "global"))
    for halo in (2, 3):
        need |= {"iv4:bwd<1,halo%d>" % halo, "iv4:bwd4<halo%d>" % halo}
        need |= {"iv56:bwd4<5,band,halo%d>" % halo, "iv56:bwd4<6,resident,halo%d>" % halo}
        need |= {"iv56:bwd<5,1,resident,halo%d>" % halo, "iv56:bwd<6,1,resident,halo%d>" % halo}
    need |= {"iv4:bwd<2,halo2>", "iv4:bwd<3,halo2>", "iv4:band"}
    need |= {"iv56:bwd<5,2,resident,halo2>", "iv56:bwd<5,3,memory,halo2>", "iv56:bwd<6,2,resident,halo2>", "iv56:bwd<6,3,resident,halo2>"}
    need |= {"iv56:fwd<5,1,lds>", "iv56:fwd<6,4,lds>", "iv56:fwd<5,4,global>"}
    need |= {"iv4:gx_tile", "iv4:gx_memory", "iv56:gx_tile", "iv56:gx_memory"}
    return need


# --------------------------------------------------------------------------------------------------------------------- the arena
class Arena(object):
    """Byte layout of one allocation that holds every buffer of a call.  add(name, nbytes, kind, mod, rem): the buffer starts at
    the first offset after the previous buffer's slack with offset % mod == rem; kind 'out' (slack = FILL bytes), 'in' (slack = NaN
    floats, laid on the buffer's own 4-byte grid) or 'mask_in' (slack = all-ones).  The allocation's base must be 16-byte aligned."""

    def __init__(self):
        self.items, self.size = {}, 0

    def add(self, name, nbytes, kind, mod=16, rem=0):
        assert kind in ("in", "out", "mask_in") and name not in self.items
        off = self.size + SLACK
        off += (rem - off) % mod
        self.items[name] = (off, int(nbytes), kind)
        self.size = off + int(nbytes) + SLACK
        return self

    def image(self, contents):
        """the arena's initial bytes: contents[name] (any array of the buffer's size in bytes) inside, the kind's slack around"""
        img = np.zeros(self.size, np.uint8)
        for name, (off, n, kind) in self.items.items():
            lo = off - SLACK
            if kind == "out":
                img[lo:off] = FILL
                img[off + n:off + n + SLACK] = FILL
            elif kind == "mask_in":
                img[lo:off] = 0xFF
                img[off + n:off + n + SLACK] = 0xFF
            else:
                nan = np.frombuffer(np.full(SLACK // 4 + 1, np.nan, np.float32).tobytes(), np.uint8)
                img[off - SLACK:off] = nan[:SLACK]
                tail = (-n) % 4                          # keeps the NaN on the grid of the buffer's floats
                img[off + n:off + n + SLACK] = np.roll(nan[:SLACK + 4], tail)[4:SLACK + 4] if tail else nan[:SLACK]
            b = np.ascontiguousarray(contents[name]).view(np.uint8).reshape(-1)
            assert b.size == n, (name, b.size, n)
            img[off:off + n] = b
        return img

    def offset(self, name):
        return self.items[name][0]

    def get(self, img, name, dtype):
        off, n, _ = self.items[name]
        return img[off:off + n].copy().view(dtype)

    def outside_changed(self, before, after, written):
        """names of the buffers whose slack changed, plus the buffers not in `written` whose content changed"""
        bad = []
        for name, (off, n, _) in self.items.items():
            if not (np.array_equal(before[off - SLACK:off], after[off - SLACK:off]) and
                    np.array_equal(before[off + n:off + n + SLACK], after[off + n:off + n + SLACK])):
                lo = np.flatnonzero(before[off - SLACK:off] != after[off - SLACK:off]) - SLACK
                hi = np.flatnonzero(before[off + n:off + n + SLACK] != after[off + n:off + n + SLACK])
                bad.append("slack of %s changed (bytes %s before the buffer, %s after it)" % (name, lo[:8].tolist(), hi[:8].tolist()))
            if name not in written and not np.array_equal(before[off:off + n], after[off:off + n]):
                bad.append("%s is an input and was changed" % name)
        return bad


def stage_arena(case, k, backward, with_mask):
    """the buffers of one stage call at float offset k: x, wq<m>, then out (+ inside) or gout (+ inside), gw<m>, gx.
    `inside` sits 2 bytes past a 4-byte boundary."""
    B, C, H, W = case.shape
    u, rows = case.u, rows_of(case.interval)
    a = Arena()
    a.add("x", 4 * B * C * H * W, "in", 16, k)
    for m in range(case.M):
        a.add("wq%d" % m, 4 * rows * u * u, "in", 16, k)
    if backward:
        a.add("gout", 4 * B * C * H * W * u * u, "in", 16, k)
        if with_mask:
            a.add("inside", 2 * B * C * H * W, "mask_in", 4, 2)
        for m in range(case.M):
            a.add("gw%d" % m, 4 * rows * u * u, "out", 16, k)
        a.add("gx", 4 * B * C * H * W, "out", 16, k)
    else:
        a.add("out", 4 * B * C * H * W * u * u, "out", 16, k)
        if with_mask:
            a.add("inside", 2 * B * C * H * W, "out", 4, 2)
    return a


# ------------------------------------------------------------------------------------------------------------------ accumulation
def prefill(case, salt=0):
    """seeded numerators (int64) for every element of every grad_wq and of grad_x: about a third zero, the rest in +-PREFILL"""
    rng = np.random.default_rng(zlib.crc32(("prefill%d_" % salt + case.name).encode()))
    rows, el = rows_of(case.interval), case.u * case.u

    def draw(shape):
        v = rng.integers(-PREFILL, PREFILL + 1, shape)
        return np.where(rng.random(shape) < 0.3, 0, v)
    return [draw((rows, el)) for _ in range(case.M)], draw(case.shape)


def gx_bound(case):
    """an upper bound of sum |terms| * q over the elements of grad_x, from the case alone: a pass hands d/d f of each of its four
    keys to that key's pixel, a term g . (p_j - p_{j-1}) with |p_j - p_{j-1}| <= 254 per element, so a pixel collects at most
    254 * sum |g| of every (site, pass, key) that reads it -- counted here by running the oracle's own gather (ft_exact_cases._passes,
    replicate padding and rotations included) on an image of pixel numbers"""
    B, C, H, W = case.shape
    assert B <= fx.REACH_BATCH
    shadow = copy.copy(case)
    shadow.x = np.arange(B * C * H * W, dtype=np.float32).reshape(case.shape)
    u = case.u
    g = (np.abs(case.gout.astype(np.float64)) / case.avg).reshape(B, C, H, u, W, u).sum((3, 5))
    acc = np.zeros(B * C * H * W)
    with fw.wide_oracle():
        for _, _, v in fx._passes(shadow):
            for k in range(4):
                np.add.at(acc, v[..., k].reshape(-1), g.reshape(-1))
    return int(np.ceil(acc.max() * 254))


def accumulate_cap(case, ref, calls=2):
    """the largest sum of magnitudes, times q, that a partial sum of `calls` backward calls into prefilled buffers can reach, over
    grad_wq (ref.cap: the oracle's own sum |terms|) and grad_x: below 2^24 every float32 partial sum is exact in any order"""
    return calls * max(ref.cap, gx_bound(case)) + PREFILL


def as_f32(num, q):
    v = (np.asarray(num, np.float64) / q).astype(np.float32)
    assert np.array_equal(v.astype(np.float64) * q, num)
    return v


# ------------------------------------------------------------------------------------------------------------------ the quantiser
QUANT_N = (1, 255, 257, 6561 * 16)
QUANT_M = (1, 3, 8)

# mulut_eval_y: one window; a second tile of one column (11 x 43) and of one row (43 x 11)
EVAL_SHAPES = ((11, 11), (11, 43), (43, 11))
EVAL_SHAVES = (0, 5)


# ---------------------------------------------------------------------------------------------------------------------- the clamp
BAD_VALUES = (-300.0, -1.0, -0.5, 255.5, 256.0, 1e9, np.inf, -np.inf, np.nan)


def f32_bits(pattern):
    return np.array([pattern], np.uint32).view(np.float32)[0]


NEG_NAN = f32_bits(0xFFC00000)           # a NaN with its sign bit set (what 0 * inf or inf - inf gives on an x86 host)
NEG_DENORMAL = f32_bits(0x80000001)      # -2^-149: its quotient by q underflows to -0, so its LSB is the negative denormal itself
# Mixed bad values within one pass, the anchor at MSB 15: with an LSB whose sign bit is set the six comparisons of the rank code can
# form a cycle, one key's stride is then added twice, and from MSB 15 that row lies past the table.  A 4 x 4 block of these is written
# into the poisoned cases, so that under every pattern and rotation some pass reads 255 next to a sign-set LSB.
BAD_BLOCK = np.array([[255.0, NEG_NAN, 255.0, NEG_DENORMAL],
                      [np.nan, 0.0, 0.0, 8.0],
                      [255.0, NEG_DENORMAL, 255.0, NEG_NAN],
                      [0.0, 8.0, np.nan, 0.0]], np.float32)
CLAMP_SHAPE = (1, 2, 24, 22)
CLAMP_CASES = [
    fx.Case(4, 1, 0, "sdy", CLAMP_SHAPE, "noise"),               # ft_stage_fwd<1>, ft_stage_bwd<1, 2>
    fx.Case(4, 4, 1, "sdy", CLAMP_SHAPE, "noise"),               # ft_stage_fwd<4>, ft_stage_bwd4<2>
    fw.WideCase(4, 1, 0, "eho", CLAMP_SHAPE, "noise"),           # ft_stage_bwd<1, 3>: a halo-3 instance
]
# stream order and capture: one case per family, and for the capture a second content of the same shape (another draw of the seed)
FAMILY_CASES = {
    "iv4_u1": _pick(CASES, interval=4, u=1, last=0, modes="sdy", shape=(1, 2, 9, 11)),
    "iv4_u4": _pick(CASES, interval=4, u=4, last=1, modes="sdy", shape=(2, 1, 13, 10)),
    "iv5_u4": _pick(CASES, interval=5, u=4, last=1, modes="sdy", shape=(2, 1, 13, 10)),
    "iv6_u2": _pick(CASES, interval=6, u=2, last=1, modes="sdy", shape=(2, 1, 13, 10)),
    "wide": _pick(CASES, interval=4, u=4, modes="sdyeho", shape=(2, 1, 13, 10)),
}
FAMILY_ENTRY = {"iv4_u1": "mask", "iv4_u4": "mask", "iv5_u4": "interval", "iv6_u2": "interval", "wide": "wide"}
SECOND = {k: fw.WideCase(c.interval, c.u, c.last, c.modes, c.shape, c.content, draw=7) for k, c in FAMILY_CASES.items()}
EXTRA = CLAMP_CASES + list(SECOND.values())


def bad_pixels(case):
    """[(plane, y, x, value)]: one pixel per BAD_VALUES entry -- the four corners of the first plane and the last pixel of the last
    among them, the rest seeded, no two within the same row"""
    B, C, H, W = case.shape
    rng = np.random.default_rng(zlib.crc32(("bad_" + case.name).encode()))
    fixed = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (B * C - 1, H - 1, W - 1)]
    ys = rng.permutation(np.arange(2, H - 2))[:len(BAD_VALUES) - len(fixed)]
    seeded = [(int(rng.integers(0, B * C)), int(y), int(rng.integers(0, W))) for y in ys]
    order = rng.permutation(len(BAD_VALUES))
    return [pos + (BAD_VALUES[i],) for pos, i in zip(fixed + seeded, order)]


def poisoned(case):
    """(x with the bad pixels and BAD_BLOCK written in, sites [B, C, H, W] bool that read one of them under some mode and rotation, the
    pixels [B, C, H, W] bool that were written): a site reads pixels up to `halo` away in either axis, replicate padding included (a
    clamped coordinate is never farther than the offset)"""
    B, C, H, W = case.shape
    x = case.x.copy().reshape(B * C, H, W)
    hit = np.zeros((B * C, H, W), bool)
    changed = np.zeros((B * C, H, W), bool)
    r = halo_of(case)
    for pl, y, xx, v in bad_pixels(case):
        x[pl, y, xx] = v
        changed[pl, y, xx] = True
        hit[pl, max(0, y - r):y + r + 1, max(0, xx - r):xx + r + 1] = True
    pl, y0, x0 = B * C - 1, H // 2 - 2, W // 2 - 2
    x[pl, y0:y0 + 4, x0:x0 + 4] = BAD_BLOCK
    changed[pl, y0:y0 + 4, x0:x0 + 4] = True
    hit[pl, y0 - r:y0 + 4 + r, x0 - r:x0 + 4 + r] = True
    return x.reshape(case.shape), hit.reshape(case.shape), changed.reshape(case.shape)
