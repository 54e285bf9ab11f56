"""Shared builders and reach measures of tests/test_reach_cpu.py and tests/test_gpu_reach.py (TEST ONLY; NumPy and oracle/ alone).

Random int8 tables make a stage's sum collapse towards its mean: the stages after the first then read a thin diagonal slice of their
tables and the final epilogue sees the bottom of its range.  The tables built here keep every stage's input on the whole
byte range, put opposite extremes side by side, and walk the epilogue's numerator over every rounding tie; the measures below state,
from the oracle alone, what a case reaches."""
import numpy as np

from oracle import c_oracle

PATTERNS = {"s": ((0, 0), (0, 1), (1, 0), (1, 1)), "d": ((0, 0), (0, 2), (2, 0), (2, 2)), "y": ((0, 0), (1, 1), (1, 2), (2, 1)),
            "e": ((0, 0), (0, 3), (3, 0), (3, 3)), "h": ((0, 0), (2, 2), (2, 3), (3, 2)), "o": ((0, 0), (2, 2), (1, 3), (3, 1))}


def levels(interval):
    return 2 ** (8 - interval) + 1


def row_keys(interval):
    """The four key levels (a, b, c, d) of every table row, as int64 [4][L^4]."""
    L = levels(interval)
    idx = np.arange(L ** 4, dtype=np.int64)
    return np.stack([idx // L ** 3, (idx // L ** 2) % L, (idx // L) % L, idx % L])


# ---------------------------------------------------------------------------------------------
# tables: all seeded, int8 [L^4][v_num]
# ---------------------------------------------------------------------------------------------
def _ramp_base(interval, final):
    a = row_keys(interval)[0]
    q = 2 ** interval
    return (q * a) // 4 if final else q * a - 128        # q is a multiple of 4: the final ramp is exact


def ramp(interval, v_num, seed=0, final=False, offset=0, noise=40):
    """clip(q a - 128 + noise), a the row's first key (the pixel itself in every rotation), noise a seeded integer in +-40: a non-final stage
    of such tables returns its input (minus one, plus what is left of the noise).  A final stage sums its four rotations where a non-final
    one averages them, so its ramp is a quarter: clip((q a + noise) / 4)."""
    rng = np.random.default_rng([seed, interval, v_num, int(final)])
    n = rng.integers(-noise, noise + 1, (levels(interval) ** 4, v_num))
    q, a = 2 ** interval, row_keys(interval)[0][:, None]
    t = (q * a + n) // 4 + offset if final else q * a - 128 + n + offset
    return np.clip(t, -128, 127).astype(np.int8)


def sweep(interval, v_num, seed, offset, final, jitter):
    """The ramp without its wide noise, moved by `offset`, with a seeded 0 .. jitter - 1 on every entry: the stage numerator of a
    list of these tables is (d x pixel) + 4 q (sum of the offsets) + a few q of jitter, so a draw walks a window of numerators a few q
    wide across every output level, and the offsets place that window on the rounding ties."""
    rng = np.random.default_rng([seed, interval, v_num, int(final), 77])
    n = rng.integers(0, jitter, (levels(interval) ** 4, v_num)) if jitter else 0
    t = np.clip(_ramp_base(interval, final)[:, None] + offset + n, -128, 127).astype(np.int8)
    return np.ascontiguousarray(np.broadcast_to(t, (t.shape[0], v_num)))


def checker(interval, v_num, complement=False):
    """Element e of row r is 127 when e + (key sum of r) is even, else -128 (v_num 1: by row alone)."""
    par = row_keys(interval).sum(0)[:, None] + np.arange(v_num)[None, :]
    return np.where((par % 2 == 0) != complement, 127, -128).astype(np.int8)


def onehot(interval, v_num, complement=False):
    """One element of every row is 127 and the rest -128, the position moving with the row's keys (v_num 1: rows alternate)."""
    a, b, c, d = row_keys(interval)
    if v_num == 1:
        return checker(interval, 1, complement)
    pos = (a + 2 * b + 3 * c + 5 * d) % v_num
    hot = np.arange(v_num)[None, :] == pos[:, None]
    return np.where(hot != complement, 127, -128).astype(np.int8)


def ends(interval, v_num, seed=0, final=False):
    """Ramp tables whose rows with a key at level 0, 1, L - 2 or L - 1 hold seeded random extremes: a slot off by one at either rim of a
    band or a slab changes bytes."""
    L = levels(interval)
    t = ramp(interval, v_num, seed, final)
    k = row_keys(interval)
    rim = ((k <= 1) | (k >= L - 2)).any(0)
    rng = np.random.default_rng([seed, interval, v_num, 5])
    ext = np.where(rng.integers(0, 2, t.shape) == 1, 127, -128).astype(np.int8)
    t[rim] = ext[rim]
    return t


TABLE_KINDS = ("ramp", "ends", "checker", "checker_c", "onehot", "onehot_c")


def table(kind, interval, v_num, seed=0, final=False):
    if kind == "ramp":
        return ramp(interval, v_num, seed, final)
    if kind == "ends":
        return ends(interval, v_num, seed, final)
    if kind.startswith("checker"):
        return checker(interval, v_num, kind.endswith("_c"))
    if kind.startswith("onehot"):
        return onehot(interval, v_num, kind.endswith("_c"))
    raise ValueError(kind)


def cascade_luts(kind, stages, modes, scale, interval, seed=0):
    """lut_dict of a cascade: keys 's{stage}_{mode}'; a repeated mode of the list shares its table, as the library keeps one per (stage, mode).
    An ends table returns mid-grey for the lowest and highest levels (its rim rows are random extremes), so a stage behind it no longer
    sees them: the ends cascade has ramp tables in its non-final stages and ends tables in the final one, whose input then spans every
    level; non-final stages take ends tables in the single-stage cases."""
    out = {}
    for s in range(stages):
        last = s + 1 == stages
        for m in sorted(set(modes)):
            k = "ramp" if kind == "ends" and not last else kind
            out["s%d_%s" % (s + 1, m)] = table(k, interval, scale * scale if last else 1, seed + 31 * s + ord(m), last)
    return out


# ---------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------
FLAT = 64           # a multiple of q at every interval: a pass over flat pixels of this value reads one table row with weight q


def flat_patches(h, w):
    """Two 12 x 16 patches of image(flat=True), one in each half: (rows, columns) slices."""
    half = w // 2
    return (slice(4, 16), slice(24, 40)), (slice(4, 16), slice(half + 8, half + 24))


def image(h=64, w=192, c=3, seed=0, ragged=False, flat=False):
    """Left half smooth (a low-frequency field over 0 .. 255 with sigma = 2 noise), right half uniform noise; the first 16 columns of the
    smooth half are forced to <= 15 and its last 16 to >= 240 (level 0 and the closed top cell, which only pixels >= 256 - q reach).
    ragged: (h + 3, w + 5), no multiple of any tile.  flat: a patch of the constant FLAT in each half, where every pass reads single rows
    and the extremes of a checker or onehot table arrive in the accumulators undiluted."""
    if ragged:
        h, w = h + 3, w + 5
    rng = np.random.default_rng([seed, h, w, c])
    half = w // 2
    yy, xx = np.mgrid[0:h, 0:half].astype(np.float64)
    out = np.empty((h, w, c), np.uint8)
    for ch in range(c):
        acc = np.zeros((h, half))
        for _ in range(3):
            fy, fx = rng.uniform(0.2, 0.8, 2) * 2 * np.pi / max(h, half)
            acc += rng.uniform(0.3, 1.0) * np.sin(fy * yy + fx * xx + rng.uniform(0, 2 * np.pi))
        acc = (acc - acc.min()) / (acc.max() - acc.min()) * 255.0
        sm = np.clip(np.rint(acc + rng.normal(0, 2, acc.shape)), 0, 255).astype(np.int64)
        sm[:, :16] = sm[:, :16] // 16
        sm[:, half - 16:] = 240 + sm[:, half - 16:] // 16
        out[:, :half, ch] = sm
        out[:, half:, ch] = rng.integers(0, 256, (h, w - half))
    out[0, 0], out[-1, half - 1] = 0, 255
    if flat:
        for rows, cols in flat_patches(h, w):
            out[rows, cols] = FLAT
    return out


def rotation_sums(luts, modes, img_hwc, u, interval, rotations):
    """Sum over the modes of q x pass for the given driver rotations alone, int64 [C][H u][W u]: what an accumulator holds that adds up
    the list for one rotation, or for a merged pair of them."""
    chw = np.ascontiguousarray(np.asarray(img_hwc, np.uint8).transpose(2, 0, 1))
    return sum(pass_q_np(lut, chw, r, u, m, interval) for lut, m in zip(luts, modes) for r in rotations)


def halves(img):
    half = img.shape[1] // 2
    return img[:, :half], img[:, half:]


# ---------------------------------------------------------------------------------------------
# reach measures (oracle and NumPy only)
# ---------------------------------------------------------------------------------------------
def divisor_bias(M, interval, final):
    q = 2 ** interval
    d = q * M if final else 4 * q * M
    return d, (0 if final else 127 * d)


def pass_q_np(lut, img_chw, r, u, mode, interval):
    """c_oracle.pass_q restated in NumPy for any pattern of PATTERNS (the oracle takes s, d, y): the keys of pass_keys, the simplex walk in
    the order of their low bits (ties by key index), the u x u block turned back by the driver rotation.  test_reach_cpu.py holds it to
    c_oracle.pass_q on s, d, y; e, h, o differ from those in their offsets alone."""
    q, L = 2 ** interval, levels(interval)
    T = np.asarray(lut, np.int8).reshape(L ** 4, u * u).astype(np.int64)
    stride = np.array([L ** 3, L ** 2, L, 1], np.int64)
    out = []
    for plane in np.asarray(img_chw, np.uint8):
        H, W = plane.shape
        k = pass_keys(plane, mode, r)
        msb, lsb = k >> interval, k & (q - 1)
        order = np.argsort(-lsb, axis=0, kind="stable")
        f = np.take_along_axis(lsb, order, 0)
        idx = (msb * stride[:, None, None]).sum(0)
        acc = (q - f[0])[..., None] * T[idx]
        for j in range(4):
            idx = idx + stride[order[j]]
            acc += (f[j] - (f[j + 1] if j < 3 else 0))[..., None] * T[idx]
        blk = np.rot90(acc.reshape(H, W, u, u), -r, axes=(2, 3))
        out.append(blk.transpose(0, 2, 1, 3).reshape(H * u, W * u))
    return np.stack(out)


def stage_numerator(luts, modes, img_hwc, u, interval):
    """K = sum over modes and rotations of q x pass, int64 [C][H u][W u] (c_oracle.pass_q; its NumPy restatement for e, h, o)."""
    chw = np.ascontiguousarray(np.asarray(img_hwc, np.uint8).transpose(2, 0, 1))
    K = np.zeros((chw.shape[0], chw.shape[1] * u, chw.shape[2] * u), np.int64)
    for lut, m in zip(luts, modes):
        for r in range(4):
            K += c_oracle.pass_q(lut, chw, r, u, m, interval=interval) if m in "sdy" else pass_q_np(lut, chw, r, u, m, interval)
    return K


def epilogue(K, M, interval, final):
    """clip(rhe((K + bias) / d)) in integers, as HWC bytes."""
    d, bias = divisor_bias(M, interval, final)
    n = K + bias
    fl, rm = n // d, n % d
    up = (2 * rm > d) | ((2 * rm == d) & (fl % 2 == 1))
    return np.clip(fl + up, 0, 255).astype(np.uint8).transpose(1, 2, 0)


def pass_keys(plane, mode, r):
    """The four key bytes of every site of one plane for driver rotation r (edge-replicated), int64 [4][H][W]."""
    H, W = plane.shape
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for di, dj in PATTERNS[mode]:
        if r == 0:
            sy, sx = np.minimum(y + di, H - 1), np.minimum(x + dj, W - 1)
        elif r == 1:
            sy, sx = np.minimum(y + dj, H - 1), np.maximum(x - di, 0)
        elif r == 2:
            sy, sx = np.maximum(y - di, 0), np.maximum(x - dj, 0)
        else:
            sy, sx = np.maximum(y - dj, 0), np.minimum(x + di, W - 1)
        out.append(plane[sy, sx].astype(np.int64))
    return np.stack(out)


def anchor_levels(img, interval):
    """Key MSB levels the image presents as anchor (the level of the pixel itself: every pattern's first key)."""
    return set(np.unique(np.asarray(img) >> interval).tolist())


def tube_share(img_hwc, modes, interval):
    """Share of the passes (site x mode x rotation) whose four key levels differ by one at most."""
    inside = total = 0
    for ch in range(img_hwc.shape[2]):
        for m in modes:
            for r in range(4):
                k = pass_keys(img_hwc[:, :, ch], m, r) >> interval
                inside += int(((k.max(0) - k.min(0)) <= 1).sum())
                total += k[0].size
    return inside / total


def tie_targets(M, interval, final):
    """Numerators at and beside every rounding tie of the epilogue: n d + d / 2 - bias and both neighbours, for every tie between two
    output levels and for the two clip boundaries (-0.5 and 255.5).
    Not reachable, and left out: a non-final stage's quotient is 127 + (mean of 4 M q weights' worth of int8 entries) <= 254 exactly,
    so its ties 254.5 and 255.5 lie above every numerator an int8 table can give; its largest numerator, 254 d - bias, stands in."""
    d, bias = divisor_bias(M, interval, final)
    n = np.arange(-1, 256 if final else 254, dtype=np.int64)
    t = (n * d + d // 2 - bias)[:, None] + np.array([-1, 0, 1])[None, :]
    t = t.reshape(-1)
    return t if final else np.append(t, 254 * d - bias)


def missing_ties(numerators, M, interval, final):
    t = tie_targets(M, interval, final)
    return t[~np.isin(t, numerators)]


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
# (stages, scale, modes, interval): c_oracle takes s, d, y; the eho cascade is compared with the host emulator
CASCADES = [(2, 4, "sdy", 4), (2, 4, "sdysd", 4), (2, 4, "sdysdysd", 4), (4, 2, "sdy", 4), (2, 3, "sdy", 4), (2, 3, "sdysdysd", 4),
            (3, 1, "sdy", 4), (2, 4, "sdy", 5), (2, 2, "sdy", 5), (2, 4, "sdy", 6), (2, 2, "sdy", 6), (2, 4, "eho", 4)]

def cascade_image(case, ragged=False):
    """The image of a cascade case (the host emulator that stands in for the oracle on e, h, o is slow: a smaller one there)."""
    stages, scale, modes, interval = case
    h, w = (24, 128) if set(modes) & set("eho") else (64, 192)
    return image(h, w, 3, seed=stages + scale, ragged=ragged)


# The sweep's mode list per mode count.  The library keeps one table per (stage, pattern), so a repeated pattern repeats its table and
# doubles its share of the numerator: a list whose patterns all occur an even number of times (sdysdy) has even numerators only and
# cannot reach the neighbours of a tie.  Every list here holds each of s, d, y (what stage_tube2_kernel takes) and one pattern once:
# that one carries the jitter.  The wide lists are the two of test_gpu_wide_patterns.py; o occurs once in both.
SWEEP_LISTS = {1: "s", 2: "sd", 3: "sdy", 4: "sdys", 5: "sdysd", 6: "sdysds", 7: "sdysdsd", 8: "sdysdsds"}
WIDE_LISTS = ("eho", "sdyehoeh")
SWEEP_SHAPE = (48, 128)
_ORDER = "sdyeho"
_SPREADS = {}


def _spread(total, counts):
    """Integer offsets per pattern with sum(count x offset) == total, as even as they come."""
    M = sum(counts.values())
    base, rem = divmod(total, M)
    names = sorted(counts, key=_ORDER.index)
    key = (rem, tuple(counts[n] for n in names))
    if key not in _SPREADS:
        best = None
        for xs in np.ndindex(*(6,) * len(names)):
            xs = [x - 2 for x in xs]
            if sum(x * counts[n] for x, n in zip(xs, names)) == rem:
                cost = (max(abs(x) for x in xs), sum(abs(x) for x in xs), xs)
                if best is None or cost < best:
                    best = cost
        _SPREADS[key] = best[2]
    return {n: base + x for n, x in zip(names, _SPREADS[key])}


def sweep_luts(modes, interval, u, final, draw):
    """Tables of one sweep draw = (seed, total offset), per pattern: the offset is spread over the list, the pattern that occurs once
    carries the jitter (0 .. 2 for an even mode count, 0 .. 3 for an odd one: the window's middle then falls on a tie for an integer offset)."""
    seed, total = draw
    M = len(modes)
    counts = {m: modes.count(m) for m in set(modes)}
    off = _spread(total, counts)
    once = [m for m in "oheyds" if counts.get(m) == 1][0]
    return {m: sweep(interval, u * u, seed + _ORDER.index(m), off[m], final, jitter=(3 + M % 2 if m == once else 0)) for m in counts}


def sweep_tables(modes, interval, u, final, draw):
    """The same per position of the mode list, as c_oracle.stage takes them."""
    t = sweep_luts(modes, interval, u, final, draw)
    return [t[m] for m in modes]


def sweep_image(draw):
    return image(SWEEP_SHAPE[0], SWEEP_SHAPE[1], 3, seed=draw[0])


def sweep_numerators(modes, interval, scale, draw):
    """The numerators of one draw; scale 0 is a non-final stage."""
    final, u = scale > 0, max(scale, 1)
    return stage_numerator(sweep_tables(modes, interval, u, final, draw), modes, sweep_image(draw), u, interval)


# The sweep's draws per (mode list, interval, scale), scale 0 a non-final stage: (table seed, total ramp offset), found by a greedy search
# over seeds and offsets on the oracle alone (central offsets first, then the offsets that bring the closed top cell, level 0 and the two
# ends of the int8 range onto the ties left) and extended until test_reach_cpu.py's condition held: every tie and both its neighbours.  A
# stage of scale u gives u x u numerators per site, so a smaller scale needs more draws for the same ties: the draws of x3, x2 and x1 begin
# with those of x4 and go on; non-final stages need the most, and more at q = 64 (the window of a draw is a few q wide, a tie one).  The
# lists of SWEEP_LISTS run at every scale test_gpu_reach.py sweeps, the wide lists non-final and at x4 and x2.
SWEEP_DRAWS = {
    ("s", 4, 4): [(4, -2)],
    ("sd", 4, 4): [(6, -1)],
    ("sdy", 4, 4): [(7, -1), (16, -7)],
    ("sdys", 4, 4): [(9, 0), (18, -8)],
    ("sdysd", 4, 4): [(9, -1), (20, -9)],
    ("sdysds", 4, 4): [(9, -2), (32, 0)],
    ("sdysdsd", 4, 4): [(11, -1), (24, -11)],
    ("sdysdsds", 4, 4): [(11, -2), (38, 0)],
    ("s", 4, 3): [(4, -2), (21431, -2)],
    ("sd", 4, 3): [(6, -1)],
    ("sdy", 4, 3): [(7, -1), (16, -7)],
    ("sdys", 4, 3): [(9, 0), (18, -8), (24431, -4)],
    ("sdysd", 4, 3): [(9, -1), (20, -9)],
    ("sdysds", 4, 3): [(9, -2), (32, 0)],
    ("sdysdsd", 4, 3): [(11, -1), (24, -11)],
    ("sdysdsds", 4, 3): [(11, -2), (38, 0)],
    ("s", 4, 2): [(4, -2), (21421, 0)],
    ("sd", 4, 2): [(6, -1), (22421, -1)],
    ("sdy", 4, 2): [(7, -1), (16, -7), (23422, 0)],
    ("sdys", 4, 2): [(9, 0), (18, -8), (24422, 5), (24423, -3), (24425, 0)],
    ("sdysd", 4, 2): [(9, -1), (20, -9), (25421, 0), (25423, -2)],
    ("sdysds", 4, 2): [(9, -2), (32, 0), (26422, -2)],
    ("sdysdsd", 4, 2): [(11, -1), (24, -11), (27421, -4)],
    ("sdysdsds", 4, 2): [(11, -2), (38, 0)],
    ("s", 4, 1): [(4, -2), (21411, 0)],
    ("sd", 4, 1): [(6, -1), (22411, 0), (22413, 0), (22415, -1), (22418, -2)],
    ("sdy", 4, 1): [(7, -1), (16, -7), (23412, 0), (23413, -2), (23415, -3), (23417, 0), (23419, 0)],
    ("sdys", 4, 1): [(9, 0), (18, -8), (24411, 0), (24413, 4), (24414, 0), (24416, 0), (24418, -4), (24420, 0), (24422, 5), (24423, 0), (24425, -2), (24428, 1), (24430, 0), (24433, 0)],
    ("sdysd", 4, 1): [(9, -1), (20, -9), (25411, 0), (25412, -2), (25414, -1), (25417, 6), (25419, 1), (25420, 0), (25422, -3), (25427, -3)],
    ("sdysds", 4, 1): [(9, -2), (32, 0), (26412, 0), (26414, 3), (26415, 0), (26417, 0), (26419, -2), (26425, 6)],
    ("sdysdsd", 4, 1): [(11, -1), (24, -11), (27412, -1), (27413, -1), (27415, 5), (27416, -2), (27419, 1), (27420, -3), (27423, -1), (27425, 4), (27427, -1)],
    ("sdysdsds", 4, 1): [(11, -2), (38, 0), (28411, 0), (28413, 2), (28415, 0)],
    ("s", 4, 0): [(1, -1), (8, 0), (15, -2), (16, -1), (22, -2), (42, 11), (99, 0), (186, 13)],
    ("sd", 4, 0): [(1, 0), (8, 2), (11, 0), (16, 0), (21, 0), (44, 13), (163, 2), (331, 30)],
    ("sdy", 4, 0): [(1, 0), (6, 0), (11, 0), (17, -3), (23, 3), (28, 3), (33, 3), (73, 32), (279, 39), (434, 0), (683, 45)],
    ("sdys", 4, 0): [(1, 1), (8, 5), (11, 1), (18, 5), (24, 2), (28, 5), (63, 27), (320, 21), (622, 60)],
    ("sdysd", 4, 0): [(1, 1), (6, 1), (11, 1), (16, 1), (23, 6), (26, 1), (33, 6), (74, 33), (371, 3), (691, -4), (1110, 88)],
    ("sdysds", 4, 0): [(1, 2), (8, 8), (11, 2), (18, 8), (21, 2), (27, -4), (110, 74), (746, 1517)],
    ("sdysdsd", 4, 0): [(1, 2), (6, 2), (11, 2), (16, 2), (22, -5), (28, 9), (31, 2), (399, 1756), (533, 37), (978, 27), (1402, -5), (1864, 3)],
    ("sdysdsds", 4, 0): [(1, 3), (8, 11), (11, 3), (17, -5), (24, 4), (28, 11), (91, 55), (590, 35), (1083, 9), (1711, 118)],
    ("s", 5, 4): [(4, -2), (15, -2)],
    ("sd", 5, 4): [(6, -1)],
    ("sdy", 5, 4): [(6, -2), (16, -7)],
    ("sdys", 5, 4): [(7, -2), (27, 1), (35, -8)],
    ("sdysd", 5, 4): [(8, -2), (28, -1)],
    ("sdysds", 5, 4): [(9, -2), (32, 0)],
    ("sdysdsd", 5, 4): [(8, -4), (34, -1)],
    ("sdysdsds", 5, 4): [(11, -2), (38, 0)],
    ("s", 5, 3): [(4, -2), (15, -2)],
    ("sd", 5, 3): [(6, -1)],
    ("sdy", 5, 3): [(6, -2), (16, -7), (23531, -1)],
    ("sdys", 5, 3): [(7, -2), (27, 1), (35, -8), (24531, 0), (24534, 4)],
    ("sdysd", 5, 3): [(8, -2), (28, -1), (25531, 0)],
    ("sdysds", 5, 3): [(9, -2), (32, 0), (26532, 0)],
    ("sdysdsd", 5, 3): [(8, -4), (34, -1), (27532, -1), (27533, -1)],
    ("sdysdsds", 5, 3): [(11, -2), (38, 0)],
    ("s", 5, 2): [(4, -2), (15, -2), (21521, -2)],
    ("sd", 5, 2): [(6, -1), (22521, -1), (22523, -1)],
    ("sdy", 5, 2): [(6, -2), (16, -7), (23522, 0), (23525, 0)],
    ("sdys", 5, 2): [(7, -2), (27, 1), (35, -8), (24521, -4), (24524, 3), (24525, -3), (24527, 0), (24530, 1)],
    ("sdysd", 5, 2): [(8, -2), (28, -1), (25522, 0), (25523, -2), (25527, 0)],
    ("sdysds", 5, 2): [(9, -2), (32, 0), (26521, 0), (26522, -2), (26525, 0)],
    ("sdysdsd", 5, 2): [(8, -4), (34, -1), (27522, 1), (27523, -1), (27525, -2), (27527, -2)],
    ("sdysdsds", 5, 2): [(11, -2), (38, 0), (28521, -8), (28524, 0), (28525, 0)],
    ("s", 5, 1): [(4, -2), (15, -2), (21512, 1), (21513, 0)],
    ("sd", 5, 1): [(6, -1), (22511, -2), (22513, -1), (22516, 0), (22517, -1), (22519, -3), (22524, 0)],
    ("sdy", 5, 1): [(6, -2), (16, -7), (23512, 0), (23515, 0), (23516, 0), (23520, 0), (23521, 0), (23523, -2), (23526, 0), (23528, -1), (23534, -1)],
    ("sdys", 5, 1): [(7, -2), (27, 1), (35, -8), (24511, -2), (24513, 0), (24516, 1), (24518, 0), (24520, 0), (24521, 0), (24523, 0), (24524, -2), (24526, -2), (24529, 2), (24530, -5), (24534, 0), (24535, -1), (24537, -1), (24539, -4), (24543, -2), (24545, -2), (24557, -4)],
    ("sdysd", 5, 1): [(8, -2), (28, -1), (25512, 4), (25513, 0), (25515, 0), (25518, 5), (25519, 0), (25521, -4), (25524, 0), (25526, 0), (25527, 0), (25529, 0), (25531, -2), (25534, 3), (25535, 0), (25538, 3), (25542, 0), (25549, -2)],
    ("sdysds", 5, 1): [(9, -2), (32, 0), (26511, 0), (26513, 0), (26516, 0), (26517, 0), (26518, -2), (26520, -2), (26522, 0), (26524, -6), (26527, 3), (26528, 0), (26530, -2), (26534, 0), (26535, -2), (26540, -2), (26548, -3)],
    ("sdysdsd", 5, 1): [(8, -4), (34, -1), (27512, -1), (27513, -4), (27515, -1), (27518, -1), (27519, -1), (27521, -6), (27524, 5), (27525, -1), (27527, -1), (27529, -1), (27531, -1), (27533, -1), (27536, -1), (27537, -2), (27540, 7), (27542, 3)],
    ("sdysdsds", 5, 1): [(11, -2), (38, 0), (28511, 0), (28513, 0), (28516, 0), (28517, 0), (28520, 0), (28521, -2), (28525, 6), (28526, -2), (28529, -2), (28533, 0)],
    ("s", 5, 0): [(1, -1), (8, 0), (14, 0), (18, 0), (25, -2), (29, 0), (35, -2), (36, -1), (45, -2), (65, 14), (130, 8), (229, 255)],
    ("sd", 5, 0): [(2, -2), (8, 2), (11, 0), (18, 2), (21, 0), (26, 0), (33, 2), (38, 2), (41, 0), (47, -2), (85, 29), (190, -1), (324, 1), (564, 501), (622, 26)],
    ("sdy", 5, 0): [(1, 0), (8, 3), (11, 0), (18, 3), (22, -3), (27, -3), (31, 0), (38, 3), (43, 3), (47, -3), (51, 0), (60, -1), (65, -1), (115, 44), (265, 0), (466, 3), (676, 8), (863, -3), (1065, -1), (1261, -3), (1572, 765)],
    ("sdys", 5, 0): [(1, 1), (8, 5), (11, 1), (17, -3), (21, 1), (27, -3), (32, -3), (38, 5), (43, 5), (49, 2), (55, 0), (60, 0), (125, 59), (326, 5), (331, 5), (400, 61), (647, 45), (911, 46), (1272, 1020)],
    ("sdysd", 5, 0): [(1, 1), (8, 6), (13, 6), (18, 6), (22, -4), (26, 1), (32, -4), (36, 1), (42, -4), (46, 1), (52, -4), (58, 6), (65, 0), (327, 1254), (471, 73), (723, 2), (1047, 1), (1055, 2), (1383, 0), (1826, -65), (2033, 1), (2362, 6), (2689, 6), (3055, 36), (3502, -24)],
    ("sdysds", 5, 0): [(1, 2), (8, 8), (11, 2), (17, -4), (21, 2), (27, -4), (31, 2), (38, 8), (44, 3), (141, 90), (438, -4), (641, -22), (926, 88), (1224, 2), (1659, 39), (2227, 1530)],
    ("sdysdsd", 5, 0): [(1, 2), (8, 9), (13, 9), (18, 9), (22, -5), (26, 2), (31, 2), (36, 2), (43, 9), (48, 9), (52, -5), (58, 9), (61, 2), (67, -5), (75, 1), (79, 3), (191, 105), (641, 100), (1099, 103), (1464, 13), (1905, 1), (2525, -88), (3035, -33), (3523, 1785)],
    ("sdysdsds", 5, 0): [(1, 3), (8, 11), (11, 3), (17, -5), (21, 3), (27, -5), (31, 3), (38, 11), (43, 11), (48, 11), (55, 2), (179, 118), (635, 55), (1190, 91), (1737, 119), (2364, -61), (2654, 4), (3463, 2040)],
    ("s", 6, 4): [(4, -2), (15, -2)],
    ("sd", 6, 4): [(6, -1), (14, -6)],
    ("sdy", 6, 4): [(6, -2), (22, -1)],
    ("sdys", 6, 4): [(12, 3), (20, -6), (38, -5), (52, -8)],
    ("sdysd", 6, 4): [(9, -1), (20, -9), (40, -8)],
    ("sdysds", 6, 4): [(12, 1), (23, -9), (51, -2)],
    ("sdysdsd", 6, 4): [(8, -4), (36, 1), (54, -4)],
    ("sdysdsds", 6, 4): [(13, 0), (26, -12)],
    ("s", 6, 3): [(4, -2), (15, -2), (21631, 0)],
    ("sd", 6, 3): [(6, -1), (14, -6), (22631, 0)],
    ("sdy", 6, 3): [(6, -2), (22, -1), (23631, 0)],
    ("sdys", 6, 3): [(12, 3), (20, -6), (38, -5), (52, -8), (24632, 0), (24633, -1), (24636, 3), (24638, 0), (24639, -5)],
    ("sdysd", 6, 3): [(9, -1), (20, -9), (40, -8), (25632, 2), (25633, 0)],
    ("sdysds", 6, 3): [(12, 1), (23, -9), (51, -2), (26631, -2), (26634, 0)],
    ("sdysdsd", 6, 3): [(8, -4), (36, 1), (54, -4), (27632, -1)],
    ("sdysdsds", 6, 3): [(13, 0), (26, -12), (28632, 0)],
    ("s", 6, 2): [(4, -2), (15, -2), (21621, -2)],
    ("sd", 6, 2): [(6, -1), (14, -6), (22621, 0), (22624, 0), (22626, -1)],
    ("sdy", 6, 2): [(6, -2), (22, -1), (23622, -1), (23625, 3), (23626, -2), (23628, 0), (23633, -2)],
    ("sdys", 6, 2): [(12, 3), (20, -6), (38, -5), (52, -8), (24622, 4), (24623, 0), (24626, 2), (24627, 0), (24629, 0), (24631, -3), (24634, 0), (24636, 0), (24638, 0), (24639, -4), (24642, 0), (24645, -4)],
    ("sdysd", 6, 2): [(9, -1), (20, -9), (40, -8), (25622, 3), (25623, 0), (25625, -2), (25628, 0), (25629, -6), (25632, 2)],
    ("sdysds", 6, 2): [(12, 1), (23, -9), (51, -2), (26621, 0), (26624, 0), (26626, 6), (26627, 0), (26629, 0)],
    ("sdysdsd", 6, 2): [(8, -4), (36, 1), (54, -4), (27621, -4), (27623, -6), (27625, -1), (27626, -1), (27627, -1), (27630, -1), (27631, -1), (27634, 3)],
    ("sdysdsds", 6, 2): [(13, 0), (26, -12), (28621, 0), (28624, 0), (28625, -8), (28629, -2)],
    ("s", 6, 1): [(4, -2), (15, -2), (21612, 0), (21614, 1), (21615, 0), (21617, -2), (21620, 0), (21622, 0), (21624, 0)],
    ("sd", 6, 1): [(6, -1), (14, -6), (22612, 0), (22613, 0), (22614, -2), (22616, -1), (22618, 0), (22620, -3), (22622, -1), (22625, 0), (22629, 3), (22630, -1), (22632, -1), (22634, -2), (22640, -4)],
    ("sdy", 6, 1): [(6, -2), (22, -1), (23612, 0), (23613, 0), (23616, 0), (23618, 0), (23619, 0), (23621, 0), (23623, 0), (23624, 0), (23626, 0), (23627, 0), (23628, -1), (23631, 0), (23633, 0), (23636, 0), (23640, 0), (23643, 0), (23645, -2), (23648, -2), (23651, -1), (23657, -1), (23664, 0), (23668, -1)],
    ("sdys", 6, 1): [(12, 3), (20, -6), (38, -5), (52, -8), (24612, 0), (24613, 0), (24615, 0), (24617, -3), (24620, 4), (24621, 0), (24622, -3), (24624, -3), (24627, 1), (24628, 0), (24630, -2), (24632, -3), (24634, -3), (24636, -3), (24639, 3), (24641, 2), (24642, 0), (24643, -2), (24645, 0), (24648, 1), (24650, 0), (24651, 0), (24653, -5), (24655, -4), (24658, 5), (24660, 0), (24661, -2), (24664, 2), (24666, 0), (24669, -5), (24672, 0), (24673, 0), (24678, 0), (24679, -4), (24682, 0), (24684, 2), (24686, 3), (24693, -2)],
    ("sdysd", 6, 1): [(9, -1), (20, -9), (40, -8), (25611, -4), (25613, 0), (25616, 0), (25617, -2), (25620, 2), (25621, 0), (25623, 0), (25624, 0), (25627, 5), (25628, -5), (25631, -3), (25634, -1), (25636, 0), (25637, 0), (25639, -1), (25641, -4), (25643, -5), (25646, -2), (25648, -3), (25650, -2), (25653, -1), (25656, 0), (25668, 4), (25670, 0), (25671, 0), (25690, 2)],
    ("sdysds", 6, 1): [(12, 1), (23, -9), (51, -2), (26611, -6), (26613, 0), (26616, 7), (26617, -5), (26619, -5), (26622, 0), (26624, 1), (26626, 0), (26628, 0), (26630, 0), (26632, 0), (26633, -5), (26635, 0), (26637, 0), (26638, 0), (26641, 7), (26643, 1), (26645, -2), (26647, -2), (26651, 7), (26654, 0), (26655, -2), (26669, 2), (26672, -4), (26677, 0), (26680, -5)],
    ("sdysdsd", 6, 1): [(8, -4), (36, 1), (54, -4), (27611, -1), (27614, -1), (27616, 5), (27617, -1), (27620, 8), (27621, -1), (27623, -4), (27625, -1), (27627, -1), (27630, 7), (27631, -1), (27634, -1), (27635, -1), (27638, -1), (27640, -1), (27641, -1), (27644, -1), (27645, -3), (27647, -1), (27648, -8), (27650, -1), (27652, -6), (27654, -1), (27657, 3), (27658, -1), (27661, -1), (27663, -1), (27667, 5), (27668, -1), (27676, -2), (27682, -4)],
    ("sdysdsds", 6, 1): [(13, 0), (26, -12), (28612, 8), (28613, -4), (28616, 6), (28617, 0), (28620, 0), (28622, 0), (28623, -6), (28625, -2), (28627, -6), (28629, 0), (28633, 0), (28635, -2), (28637, -2), (28642, 8), (28651, -2)],
    ("s", 6, 0): [(3, 0), (9, 0), (14, 0), (16, -1), (23, 0), (26, -1), (33, 0), (40, -2), (41, -1), (49, 0), (53, 0), (60, -2), (63, 0), (69, 0), (75, -2), (77, -2), (85, -2), (87, -2), (136, 253), (166, -2), (244, 6), (322, 13), (397, 17), (503, 250)],
    ("sd", 6, 0): [(1, 0), (6, 0), (11, 0), (18, 2), (22, -2), (28, 2), (33, 2), (36, 0), (41, 0), (48, 2), (52, -2), (56, 0), (61, 0), (66, 0), (72, -2), (76, 0), (84, 1), (88, 2), (94, 1), (98, 2), (174, -4), (321, 507), (375, -1), (507, -2), (642, -2), (813, 32)],
    ("sdy", 6, 0): [(3, 3), (6, 0), (13, 3), (18, 3), (21, 0), (26, 0), (33, 3), (38, 3), (43, 3), (48, 3), (52, -3), (56, 0), (61, 0), (66, 0), (72, -3), (77, -3), (85, -1), (86, 0), (92, -3), (97, -3), (101, 0), (107, -3), (143, 27), (310, 0), (317, 3), (369, 44), (545, 21), (729, 6), (934, 12), (1275, 752), (1352, 32), (1514, 0), (1714, -3), (1914, 3), (2114, 1), (2310, 0), (2509, 0), (2708, 0), (2918, 6), (3122, 11)],
    ("sdys", 6, 0): [(3, 5), (8, 5), (12, -3), (18, 5), (21, 1), (28, 5), (32, -3), (38, 5), (43, 5), (47, -3), (54, 2), (60, 0), (61, 1), (70, 0), (71, 1), (77, -3), (85, 0), (87, -3), (94, 2), (96, 1), (164, 58), (462, -51), (765, -11), (1049, 1009), (1167, 9), (1439, 18), (1749, 65), (2006, 59), (2355, 1000)],
    ("sdysd", 6, 0): [(3, 6), (6, 1), (12, -4), (18, 6), (21, 1), (28, 6), (33, 6), (38, 6), (42, -4), (46, 1), (51, 1), (58, 6), (61, 1), (68, 6), (72, -4), (78, 6), (81, 1), (90, 0), (92, -4), (99, 2), (101, 1), (110, 0), (111, 1), (117, -4), (121, 1), (205, 74), (454, -4), (462, 0), (483, 15), (792, 6), (795, 1), (825, 20), (1315, 1252), (1525, 66), (1866, 80), (2137, 24), (2641, 1270), (2815, 48), (3205, -69), (3457, 36), (3875, -53), (4216, -39), (4400, 2), (4901, -8), (5051, 1), (5379, -4), (5705, 1), (6070, 33), (6359, 1), (7104, 86)],
    ("sdysds", 6, 0): [(3, 8), (8, 8), (12, -4), (18, 8), (21, 2), (28, 8), (32, -4), (38, 8), (43, 8), (47, -4), (54, 3), (58, 8), (65, 1), (69, 3), (74, 3), (287, -10), (678, -10), (1021, -58), (1343, 89), (1973, 1526), (2033, 8), (2422, 2), (2814, -4), (3800, -16)],
    ("sdysdsd", 6, 0): [(3, 9), (6, 2), (13, 9), (16, 2), (21, 2), (28, 9), (33, 9), (38, 9), (42, -5), (48, 9), (51, 2), (56, 2), (61, 2), (68, 9), (74, 3), (78, 9), (81, 2), (88, 9), (92, -5), (97, -5), (101, 2), (106, 2), (115, 1), (119, 3), (121, 2), (155, 24), (689, 103), (1046, 5), (1582, 86), (1997, 46), (2471, 65), (2657, 102), (2948, 87), (3312, -5), (3455, -118), (3772, -5), (3840, 59), (4618, 1780), (4881, -62), (5199, 53), (5728, -125), (6141, 85), (6540, 29), (6961, 2), (7420, 1), (7949, 73), (8338, 7), (8792, 6), (9260, 19), (9721, 25), (10196, 45), (10603, 9), (11110, 49), (12422, -5)],
    ("sdysdsds", 6, 0): [(3, 11), (8, 11), (11, 3), (18, 11), (21, 3), (28, 11), (31, 3), (38, 11), (42, -5), (49, 4), (53, 11), (58, 11), (63, 11), (70, 2), (74, 4), (356, -13), (1036, 2034), (1195, 76), (1745, 107), (2152, 3), (2795, 119), (3259, 64)],
    ("eho", 4, 4): [(23442, 0), (23445, -6)],
    ("sdyehoeh", 4, 4): [(28443, 0), (28445, -16)],
    ("eho", 4, 2): [(23422, 0), (23425, -6), (23428, -4)],
    ("sdyehoeh", 4, 2): [(28422, 0), (28425, -16)],
    ("eho", 4, 0): [(23402, 0), (23405, 765), (23406, 0), (23407, 0), (23408, 0), (23409, 0), (23410, 0), (23411, 0), (23418, 39), (23422, 24), (23429, 14), (23446, -1)],
    ("sdyehoeh", 4, 0): [(28402, 3), (28405, 2040), (28406, 3), (28407, 3), (28408, 3), (28409, 3), (28410, 3), (28413, 54), (28419, 3), (28422, 55), (28439, -4), (28483, 10), (28511, -4), (28539, 67), (28556, -3)],
    ("eho", 5, 4): [(23542, -3), (23546, 0)],
    ("sdyehoeh", 5, 4): [(28542, 0), (28545, -16)],
    ("eho", 5, 2): [(23522, -1), (23526, 0), (23527, 0), (23529, -2)],
    ("sdyehoeh", 5, 2): [(28523, 0), (28525, -16), (28528, 0)],
    ("eho", 5, 0): [(23502, 0), (23505, 765), (23506, 0), (23507, 0), (23508, 0), (23509, 0), (23510, 0), (23511, 0), (23512, 0), (23513, 0), (23514, 0), (23515, 0), (23516, 0), (23524, 84), (23531, 81), (23536, 42), (23545, 59), (23552, 49), (23561, 52), (23565, 0), (23571, 51)],
    ("sdyehoeh", 5, 0): [(28502, 3), (28505, 2040), (28506, 3), (28507, 3), (28508, 3), (28509, 3), (28510, 3), (28511, 3), (28512, 3), (28513, 3), (28514, 3), (28515, 3), (28516, 3), (28517, 3), (28521, 102), (28528, 66), (28539, 197), (28548, 243), (28556, 187), (28561, 91), (28568, 69), (28577, 123), (28583, 74), (28592, 139), (28603, 140), (28609, 176), (28616, 113), (28624, 119), (28681, 124)],
    ("eho", 6, 4): [(23642, 0), (23645, -6)],
    ("sdyehoeh", 6, 4): [(28643, 0), (28645, -16)],
    ("eho", 6, 2): [(23623, 0), (23625, -6), (23629, 3), (23630, 0), (23631, -2), (23633, -3), (23635, 0)],
    ("sdyehoeh", 6, 2): [(28622, 0), (28625, -16), (28628, -8), (28630, 0), (28632, 0)],
    ("eho", 6, 0): [(23602, 0), (23605, 765), (23606, 0), (23607, 0), (23608, 0), (23609, 0), (23610, 0), (23611, 0), (23612, 0), (23613, 0), (23614, 0), (23615, 0), (23616, 0), (23617, 0), (23618, 0), (23619, 0), (23620, 0), (23621, 0), (23622, 0), (23623, 0), (23624, 0), (23625, 0), (23626, 0), (23627, 0), (23628, 0), (23629, 0), (23630, 0), (23638, 180), (23645, 99), (23653, 130), (23660, 120), (23669, 126), (23677, 131), (23679, 0), (23680, 0), (23684, 61), (23693, 102), (23703, 153), (23710, 126), (23715, 66), (23723, 114), (23744, 2), (23762, 62), (23784, 2), (23815, 2)],
    ("sdyehoeh", 6, 0): [(28602, 3), (28605, 2040), (28606, 3), (28607, 3), (28608, 3), (28609, 3), (28610, 3), (28611, 3), (28612, 3), (28613, 3), (28614, 3), (28615, 3), (28616, 3), (28617, 3), (28618, 3), (28619, 3), (28620, 3), (28621, 3), (28629, 475), (28630, 3), (28631, 3), (28638, 415), (28643, 169), (28648, 3), (28655, 427), (28664, 411), (28670, 307), (28679, 395), (28686, 312), (28695, 418), (28702, 371), (28709, 297), (28717, 379), (28725, 390), (28731, 134), (28739, 194), (28747, 142), (28756, 293), (28764, 411), (28774, 419), (28784, 464), (28818, 510), (28833, -4), (28863, 460), (28869, 323), (28879, 403), (28884, 203), (28906, 4)],
}
