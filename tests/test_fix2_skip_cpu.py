"""The argument behind stage_up_fix2_kernel's entry-level skip, on the CPU (NumPy; the kernel's predicate compiled with g++ from
tests/host_emul/emul_fix2_skip.cpp).

A pass of the final stage weighs the table rows floor((x_i + s) / 16), i = the four pixels of the pass, for shifts s = 0 .. 16 (a
shift between two tied low nibbles has weight 0).  The tube band holds the rows whose keys span at most two steps, at the slot the tube
kernels' address arithmetic gives any row.  So a sample whose passes all have values within 32 levels is exact as the tube kernel
stored it, although its key MSBs may span two steps and put it on the fix-up list.  Bars: every row reached from a tuple within 32 levels
is in the band, the slot map is injective on them, a range of 33 reaches a span of three, and the kernel's predicate equals the
max - min definition under the kernels' row and column clamps."""
import ctypes

import numpy as np
import pytest

import fix2_cases as X
import fix2_skip_cases as S
from host_emul_lib import load_emul
from oracle import c_oracle

SHIFTS = np.arange(17)


def vertices(x):
    """[..., 17]: floor((x + s) / 16) for s = 0 .. 16"""
    return (np.asarray(x, np.int32)[..., None] + SHIFTS) >> 4


def test_every_row_within_32_levels_is_in_the_band_at_its_own_slot():
    """Every four-value tuple with max - min <= 32: the minimum 0 .. 255, the other three 0 .. 32 above it (up to 255), the minimum in each of
    the four positions -- 33.3 M tuples (37 M less those that would pass 255), none left out.  (tube_contains is symmetric in its keys, so the position of the minimum only
    matters for the set of rows reached: the rows are collected for all four.)"""
    reached = np.zeros(S.L ** 4, bool)
    tuples = exact32 = 0
    for mn in range(256):
        top = min(S.REACH, 255 - mn)
        o = np.arange(top + 1)
        vm = vertices(mn)                                   # [17]
        vo = vertices(mn + o)                               # [top + 1][17]
        a, b, c = vo[:, None, None, :], vo[None, :, None, :], vo[None, None, :, :]
        m = np.broadcast_to(vm, np.broadcast(a, b, c).shape)
        assert S.tube_contains(m, a, b, c).all(), mn
        tuples += 4 * (top + 1) ** 3
        exact32 += 4 * ((top + 1) ** 3 - top ** 3) if top == S.REACH else 0
        keys = [np.broadcast_to(k, m.shape).ravel() for k in (m, a, b, c)]
        for p in range(4):                                  # the minimum as key A, B, C, D
            k = keys[1:p + 1] + keys[:1] + keys[p + 1:]
            reached[((k[0] * S.L + k[1]) * S.L + k[2]) * S.L + k[3]] = True
    rows = np.flatnonzero(reached)
    a, b, c, d = rows // S.L ** 3, rows // S.L ** 2 % S.L, rows // S.L % S.L, rows % S.L
    slots = S.tube_slot(a, b, c, d)
    print("tuples", tuples, "of them with a range of exactly 32:", exact32, "; rows reached", len(rows), "slots", slots.min(), "..", slots.max())
    assert tuples == 4 * sum(min(33, 256 - mn) ** 3 for mn in range(256)) > 33_000_000 and exact32 == 4 * (256 - S.REACH) * (33 ** 3 - 32 ** 3)
    assert S.tube_contains(a, b, c, d).all()
    assert len(np.unique(slots)) == len(rows) and slots.min() >= 0 and slots.max() <= 1040
    # the other way round: the band has no row a tuple within 32 levels cannot reach (991 rows: mulut_core.h)
    assert len(rows) == 991


def test_the_bound_is_tight():
    """Range 33: (v, v + 33, v, v) and its permutations reach a span of three at the shift that brings v to a low nibble of 15, for every v.
    So does every tuple with a range of 33 (sampled: the two extremes and two values between them)."""
    rng = np.random.default_rng(33)
    for v in range(256 - 33):
        for p in range(4):
            t = [v] * 4
            t[p] = v + 33
            keys = vertices(np.array(t))                    # [4][17]
            span = keys.max(0) - keys.min(0)
            assert span.max() == 3 and not S.tube_contains(*keys[:, span.argmax()]), (v, p)
    lo = rng.integers(0, 256 - 33, 20000)
    mid = lo[:, None] + rng.integers(0, 34, (20000, 2))
    keys = vertices(np.concatenate([lo[:, None], mid, lo[:, None] + 33], axis=1))      # [n][4][17]
    assert ((keys.max(1) - keys.min(1)).max(1) == 3).all()


@pytest.fixture(scope="module")
def lib():
    lb = load_emul("emul_fix2_skip", ["mulut_core.h"])
    lb.fix2_far_map.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3
    lb.fix2_far_map.restype = None
    lb.fix2_reach.restype = ctypes.c_int
    return lb


def twin_far(lib, plane, modes, rows):
    H, W = plane.shape
    di = np.ascontiguousarray([[d[0] for d in X.PAT[m]] for m in modes], np.int32)
    dj = np.ascontiguousarray([[d[1] for d in X.PAT[m]] for m in modes], np.int32)
    far = np.zeros((rows[1] - rows[0], W), np.uint16)
    plane = np.ascontiguousarray(plane, np.uint8)
    lib.fix2_far_map(plane.ctypes.data, H, W, rows[0], rows[1], len(modes), di.ctypes.data, dj.ctypes.data, far.ctypes.data)
    return far


@pytest.mark.parametrize("modes", ["sdy", "s", "sd", "sdys"])
def test_the_kernels_predicate_is_max_minus_min_under_its_clamps(lib, modes):
    """Lane by lane (lane = mode x rotation, in list order) on the frames of the GPU test, whole and in the strips (0, 5), (5, 6), (6, 21):
    neighbours clamped to the rows the launch holds and to columns 0 and W - 1.  The lanes beyond 4 M vote "not far"."""
    assert lib.fix2_reach() == S.REACH
    x = S.frames(*S.SHAPES[0], 1)[..., 0]
    n_far = n_near = 0
    for f in x:
        for rows in ((0, X.H),) + X.STRIPS:
            got = twin_far(lib, f, modes, rows)
            for ln in range(16):
                bit = ((got >> ln) & 1).astype(bool)
                if ln >= 4 * len(modes):
                    assert not bit.any()
                    continue
                want = S.pass_ranges(f[..., None], modes[ln >> 2], rows)[ln & 3, rows[0]:rows[1], :, 0] > S.REACH
                assert np.array_equal(bit, want), (modes, rows, ln)
                n_far, n_near = n_far + int(want.sum()), n_near + int((~want).sum())
    print(modes, "passes far", n_far, "near", n_near)
    assert n_far > 1000 and n_near > 1000


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("c", [1, 2, 3])
def test_frames_hold_both_kinds_and_a_wrong_skip_would_show(shape, c):
    """The frames of the GPU test on the oracle alone, random final tables: a few hundred flagged samples the kernel may skip and a few hundred
    it may not; with band-aliased tables (what a tube kernel stores for a flagged sample; free slots filled with -128 and with 127) the
    skippable samples keep the oracle's bytes exactly, and the flagged samples with a pass at a range of exactly 33 do not."""
    x = S.frames(*shape, c)
    tables = X.final_tables(X.luts("sdy", "random"), "sdy")
    skip = keep = shows33 = 0
    for f in x:
        fl, far = S.flagged_mask(f, "sdy"), S.far_mask(f, "sdy")
        rng = S.pass_ranges(f, "sdy")
        only33 = fl & (rng.max(0) == S.REACH + 1)
        want = c_oracle.stage(tables, "sdy", True, f, 4)
        blocks = lambda img: img.reshape(f.shape[0], 4, f.shape[1], 4, c).transpose(0, 2, 4, 1, 3)      # noqa: E731  [H][W][C][4][4]
        differs = np.ones(f.shape, bool)
        for fill in (-128, 127):
            got = c_oracle.stage(S.aliased(tables, fill), "sdy", True, f, 4)
            d = (blocks(got) != blocks(want)).any((3, 4))
            assert not d[~far].any()                     # within 32 levels the band gives the oracle's bytes, flagged or not
            differs &= d
        skip, keep, shows33 = skip + int((fl & ~far).sum()), keep + int((fl & far).sum()), shows33 + int((differs & only33).sum())
    print(shape, "C", c, "flagged and skippable", skip, "flagged and not", keep, "range-33 samples a wrong skip would show at", shows33)
    assert skip >= 200 and keep >= 200 and shows33 >= 20
