"""What the cases of tests/test_gpu_reach.py reach, asserted on the oracle alone (no GPU): a GPU comparison says nothing about table rows
no sample reads, numerators no epilogue sees or fields no extreme fills, so every condition that makes those cases meaningful is an
assert here -- on c_oracle / NumPy results only.  Random tables meet none of them."""
import numpy as np
import pytest

import reach_cases as R
from oracle import c_oracle
from test_core_math_cpu import emul, run_emul  # noqa: F401  (host emulator of mulut_core.h)
from test_interval_cpu import emul_iv, run_emul_iv  # noqa: F401  (host emulator of mulut_interval.h)


def stage_inputs(luts, stages, modes, scale, interval, img, stage_fn):
    """The input of every stage of the cascade, first to last, and its output."""
    cur, seen = img, []
    for s in range(stages):
        last = s + 1 == stages
        seen.append(cur)
        cur = stage_fn([luts["s%d_%s" % (s + 1, m)] for m in modes], modes, last, cur, scale if last else 1, interval)
    return seen, cur


def oracle_stage(luts, modes, last, img, u, interval):
    return c_oracle.stage(luts, modes, last, img, u, interval=interval)


# ---------------------------------------------------------------------------------------------
# the numerator the measures are stated on is the oracle's
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", [4, 5, 6])
def test_numerator_and_epilogue_restate_the_oracle_stage(interval):
    img = R.image(24, 64, 3, seed=1)
    for final, u in ((False, 1), (True, 4), (True, 3), (True, 1)):
        for M in (1, 3, 7, 8):
            modes = R.SWEEP_LISTS[M]
            luts = [R.ramp(interval, u * u, 7 * "sdy".index(m), final) for m in modes]
            K = R.stage_numerator(luts, modes, img, u, interval)
            assert np.array_equal(R.epilogue(K, M, interval, final), c_oracle.stage(luts, modes, final, img, u, interval=interval)), (final, u, M)


# ---------------------------------------------------------------------------------------------
# cascades: every stage's input presents every anchor level, and both regimes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ramp", "ends"])
@pytest.mark.parametrize("stages,scale,modes,interval", R.CASCADES)
def test_every_stage_of_a_cascade_sees_every_level(emul, kind, stages, scale, modes, interval):  # noqa: F811
    L, q = R.levels(interval), 2 ** interval
    wide = bool(set(modes) & set("eho"))
    fn = (lambda t, m, last, im, u, iv: run_emul(emul, t, m, last, im, u)) if wide else oracle_stage
    luts = R.cascade_luts(kind, stages, modes, scale, interval)
    for ragged in (False, True):
        img = R.cascade_image((stages, scale, modes, interval), ragged)
        seen, out = stage_inputs(luts, stages, modes, scale, interval, img, fn)
        for s, cur in enumerate(seen):
            # anchors are byte >> interval = 0 .. L - 2; level L - 1 is read as the upper vertex of the closed top cell
            assert R.anchor_levels(cur, interval) == set(range(L - 1)), (s, sorted(R.anchor_levels(cur, interval)))
            assert (cur >= 256 - q).any() and (cur < q).any(), s
            smooth, noisy = R.halves(cur)
            assert R.anchor_levels(noisy, interval) == set(range(L - 1)), s
            if interval == 4 and not wide:          # the tube band exists at interval 4, for s, d, y
                assert R.tube_share(smooth, modes, 4) >= 0.90, (s, R.tube_share(smooth, modes, 4))
                assert R.tube_share(noisy, modes, 4) <= 0.10, (s, R.tube_share(noisy, modes, 4))
        if kind == "ramp":      # the final epilogue sees its whole range unclipped: bytes from 0 / 1 up to 250 and more, most levels between
            assert out.min() <= 1 and out.max() >= 250 and len(np.unique(out)) >= 240, (out.min(), out.max(), len(np.unique(out)))


def test_detailed_tile_case_spans_the_sixteen_anchors_outside_the_tube():
    """The final stage of the 2-stage sdy x4 cascade: in the noisy half of its input every anchor MSB has samples whose pass leaves the tube
    (those are the samples the anchor-slab path takes), for each of the sixteen slab pairs."""
    for kind in ("ramp", "ends"):
        luts = R.cascade_luts(kind, 2, "sdy", 4, 4)
        img = R.image(seed=6)
        seen, _ = stage_inputs(luts, 2, "sdy", 4, 4, img, oracle_stage)
        noisy = R.halves(seen[1])[1]
        for ch in range(3):
            plane = noisy[:, :, ch]
            out_of_tube = np.zeros(plane.shape, bool)
            for m in "sdy":
                for r in range(4):
                    k = R.pass_keys(plane, m, r) >> 4
                    out_of_tube |= (k.max(0) - k.min(0)) > 1
            assert set(np.unique(plane[out_of_tube] >> 4).tolist()) == set(range(16)), (kind, ch)


# ---------------------------------------------------------------------------------------------
# the epilogue sweep reaches every tie and both its neighbours
# ---------------------------------------------------------------------------------------------
SWEEP_SCALES = {4: (0, 4, 3, 2, 1), 5: (0, 4, 3, 2, 1), 6: (0, 4, 3, 2, 1)}      # 0: non-final


def test_the_sweep_has_draws_for_every_list_interval_and_scale():
    want = {(R.SWEEP_LISTS[M], iv, sc) for iv, scs in SWEEP_SCALES.items() for sc in scs for M in range(1, 9)}
    want |= {(modes, iv, sc) for modes in R.WIDE_LISTS for iv in (4, 5, 6) for sc in (0, 4, 2)}
    assert set(R.SWEEP_DRAWS) == want


@pytest.mark.parametrize("modes,interval,scale", sorted(R.SWEEP_DRAWS), ids=lambda v: str(v))
def test_sweep_draws_reach_every_tie_and_its_neighbours(modes, interval, scale):
    """No exceptions but the proven one (reach_cases.tie_targets): a float epilogue can only go wrong at or beside a tie.  Asserted for
    every scale the GPU sweep runs (x4, x3, x2, x1 and non-final), each on its own draws, and for the wide lists with the NumPy
    restatement of the pass (test_numpy_pass_restates_the_oracle_pass)."""
    draws, M, final = R.SWEEP_DRAWS[(modes, interval, scale)], len(modes), scale > 0
    left = R.tie_targets(M, interval, final)
    assert len(left) == 3 * (257 if final else 255) + (0 if final else 1)
    lo = hi = None
    for draw in draws:
        K = R.sweep_numerators(modes, interval, scale, draw)
        left = left[~np.isin(left, K)]
        lo, hi = (K.min() if lo is None else min(lo, K.min())), (K.max() if hi is None else max(hi, K.max()))
    assert left.size == 0, (len(draws), left[:12])
    d, bias = R.divisor_bias(M, interval, final)
    assert lo + bias < -d // 2 and (hi + bias > 255 * d + d // 2 if final else hi + bias == 254 * d)      # both clips are crossed (final), the top is met (non-final)


@pytest.mark.parametrize("interval", [4, 5, 6])
def test_numpy_pass_restates_the_oracle_pass(interval):
    """pass_q_np gives c_oracle.pass_q's numbers for s, d, y at every rotation and scale; e, h, o go through the same lines with other offsets."""
    img = R.image(13, 64, 3, seed=3, ragged=True)
    chw = np.ascontiguousarray(img.transpose(2, 0, 1))
    for u in (1, 2, 3, 4):
        t = np.random.default_rng([interval, u]).integers(-128, 128, (R.levels(interval) ** 4, u * u)).astype(np.int8)
        for m in "sdy":
            for r in range(4):
                assert np.array_equal(R.pass_q_np(t, chw, r, u, m, interval), c_oracle.pass_q(t, chw, r, u, m, interval=interval)), (u, m, r)


@pytest.mark.parametrize("modes", R.WIDE_LISTS)
def test_wide_numerators_give_the_host_emulators_bytes(emul, emul_iv, modes):  # noqa: F811
    """The epilogue of the NumPy numerator of a wide list is what the host emulator writes: the reach of the wide sweep is stated on it."""
    for (mo, interval, scale), draws in sorted(R.SWEEP_DRAWS.items()):
        if mo != modes:
            continue
        final, u, draw = scale > 0, max(scale, 1), draws[-1]
        luts, img = R.sweep_tables(modes, interval, u, final, draw), R.sweep_image(draw)[:20]
        K = R.stage_numerator(luts, modes, img, u, interval)
        got = run_emul(emul, luts, modes, final, img, u) if interval == 4 else run_emul_iv(emul_iv, luts, modes, final, img, u, interval)
        assert np.array_equal(R.epilogue(K, len(modes), interval, final), got), (interval, scale)


def test_a_list_of_doubled_patterns_has_even_numerators_only():
    """Why the sweep's lists are not prefixes of sdysdysd: with every pattern twice the numerator is even, and a tie's neighbours are odd."""
    img = R.image(16, 64, 3, seed=2)
    t = {m: R.ramp(4, 1, ord(m)) for m in "sdy"}
    K = R.stage_numerator([t[m] for m in "sdysdy"], "sdysdy", img, 1, 4)
    assert (K % 2 == 0).all()
    assert (R.tie_targets(6, 4, False)[:-1].reshape(-1, 3)[:, [0, 2]] % 2 == 1).all()
    for M, modes in R.SWEEP_LISTS.items():
        assert len(modes) == M and min(modes.count(m) for m in set(modes)) == 1 and (M < 3 or set(modes) == set("sdy"))


# ---------------------------------------------------------------------------------------------
# checker and onehot tables: opposite extremes in adjacent fields of the packed accumulators
# ---------------------------------------------------------------------------------------------
def _opposite(f0, f1):
    return ((f0 == 255) & (f1 == 0)) | ((f0 == 0) & (f1 == 255))


def _tube_rows(interval=4):
    k = R.row_keys(interval)
    return (k.max(0) - k.min(0)) <= 2


def test_checker_and_onehot_put_opposite_extremes_in_adjacent_fields():
    """The field layouts, restated (mulut_capi.hip tube_band / slab_pairs; fields hold value + 128):
    x4 tube band  dword halves (e[4k], e[4k+2]) in the low plane and (e[4k+1], e[4k+3]) in the high plane;
    x4 slab rows  16 bytes e0 .. e15, two rows (A, A + 1) side by side: byte neighbours (e, e + 1), and e15 of row A next to e0 of row A + 1;
    x3 tube band  ten fields e0 e1 e2 e3 e4 e4 e5 e6 e7 e8, dwords of two;  x2: (e0, e1), (e2, e3);
    1-byte rows   the value in both halves of a dword: extremes meet between the rows a pass adds up."""
    tube = _tube_rows()
    for comp in (False, True):
        ch, oh = R.checker(4, 16, comp).astype(int) + 128, R.onehot(4, 16, comp).astype(int) + 128
        # x4 tube band: the checker fills both halves of a dword alike (e and e + 2 share their parity) -- every field at the same extreme,
        # rows alternating; the onehot rows put 255 next to 0 (or 0 next to 255) in exactly one dword of every row of the band
        pairs = [(4 * k + p, 4 * k + p + 2) for k in range(4) for p in (0, 1)]
        assert not any(_opposite(ch[tube][:, a], ch[tube][:, b]).any() for a, b in pairs)
        n_opp = sum(_opposite(oh[tube][:, a], oh[tube][:, b]).astype(int) for a, b in pairs)
        assert (n_opp == 1).all() and tube.sum() == 991
        for a, b in pairs:                                   # and every dword of the slot takes its turn
            assert _opposite(oh[tube][:, a], oh[tube][:, b]).any(), (a, b)
        # x4 slab rows: byte neighbours
        assert all(_opposite(ch[:, e], ch[:, e + 1]).all() for e in range(15))
        assert (sum(_opposite(oh[:, e], oh[:, e + 1]).astype(int) for e in range(15)) >= 1).all()
        nxt = np.arange(17 ** 4 - 17 ** 3) + 17 ** 3          # row (A + 1, b, c, d) of row (A, b, c, d)
        assert _opposite(ch[:-17 ** 3, 0], ch[nxt, 0]).all()  # the pair's two rows are complements, element by element
        # x3: dwords (e0,e1) (e2,e3) (e4,e4) (e5,e6) (e7,e8); x2: (e0,e1) (e2,e3)
        c9, o9 = R.checker(4, 9, comp).astype(int) + 128, R.onehot(4, 9, comp).astype(int) + 128
        f9 = lambda t: np.stack([t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4], t[:, 4], t[:, 5], t[:, 6], t[:, 7], t[:, 8]], 1)  # noqa: E731
        for t, dwords in ((f9(c9), (0, 1, 3, 4)), (R.checker(4, 4, comp).astype(int) + 128, (0, 1))):
            for k in range(t.shape[1] // 2):
                assert _opposite(t[:, 2 * k], t[:, 2 * k + 1]).all() == (k in dwords), k
        assert (sum(_opposite(f9(o9)[:, 2 * k], f9(o9)[:, 2 * k + 1]).astype(int) for k in range(5)) >= (o9[:, 4] != (0 if comp else 255))).all()
    # rows one step apart in one key are complements (the simplex walk adds them up with weights that sum to q): 1-byte rows too
    for iv in (4, 5, 6):
        L, c1 = R.levels(iv), R.checker(iv, 1).astype(int)[:, 0]
        for stride in (1, L, L * L, L ** 3):
            k = R.row_keys(iv)[{1: 3, L: 2, L * L: 1, L ** 3: 0}[stride]]
            ok = k < L - 1
            assert (c1[:-stride][ok[:-stride]] + c1[stride:][ok[:-stride]] == -1).all()


@pytest.mark.parametrize("M", [1, 3, 4, 8])
def test_accumulated_fields_hold_opposite_extremes_side_by_side(M):
    """The same on what a kernel accumulates, not on table rows: the numerators of the x4 final stage on image(flat=True), inside its flat
    patches (two sites in from their edge, so that every key of every pattern is the constant).  Measured on the oracle:
    one rotation, the list summed: checker puts +127 q M beside -128 q M in every pair of byte neighbours (e, e + 1) and the same extreme in
      both dword halves (e, e + 2); onehot puts its hot element at +127 q M beside -128 q M in its dword partner (e + 2) and in both byte
      neighbours -- true opposite extremes, in every accumulator that adds up one rotation;
    all four rotations (the stage numerator): the block turns with the rotation, so no element is hot, or 127, in all four.  onehot reaches
      the bottom rim -128 x 4 q M (K = -32768 at M = 4, -65536 at M = 8) beside fields that differ (a hot element adds 255 q M), its
      complement the top rim 127 x 4 q M; checker's four rotations cancel to -2 q M everywhere.  A full-swing pair of numerators summed
      over all four rotations does not occur with these tables: opposite extremes meet per rotation and per merged pair of rotations."""
    q, modes = 16, R.SWEEP_LISTS[M]
    img = R.image(48, 128, 3, seed=M, flat=True)[:20]          # the patches and their surroundings: rows 4 .. 15
    top, bot = 127 * q * M, -128 * q * M
    for rows, cols in R.flat_patches(48, 128):
        inner = (slice(None), slice(4 * (rows.start + 3), 4 * (rows.stop - 3)), slice(4 * (cols.start + 3), 4 * (cols.stop - 3)))
        for comp in (False, True):
            hot, cold = (bot, top) if comp else (top, bot)
            ch = [R.checker(4, 16, comp)] * M
            oh = [R.onehot(4, 16, comp)] * M
            for r in range(4):          # (an odd rotation turns the block's rows into output columns: the element's neighbours lie along y)
                turn = (lambda a: a.transpose(0, 2, 1)) if r % 2 else (lambda a: a)
                P = turn(R.rotation_sums(ch, modes, img, 4, 4, (r,))[inner])
                assert set(np.unique(P).tolist()) == {top, bot}
                assert (P[:, :, :-1] + P[:, :, 1:] == top + bot).all()            # byte neighbours: opposite extremes
                assert (P[:, :, :-2] == P[:, :, 2:]).all()                        # dword halves: the same extreme
                P = turn(R.rotation_sums(oh, modes, img, 4, 4, (r,))[inner])
                ys, xs = np.nonzero(P[0] == hot)
                assert len(ys) == P[0].size // 16 and set(np.unique(P).tolist()) == {top, bot}
                for dx in (-2, -1, 1, 2):           # the hot field's dword partner and byte neighbours, inside its own block or the next
                    ok = (xs + dx >= 0) & (xs + dx < P.shape[2])
                    assert (P[0][ys[ok], xs[ok] + dx] == cold).all()
            for pair in ((0, 1), (2, 3), (0, 2)):                                 # a merged pair of rotations: a rim beside the middle
                P = R.rotation_sums(ch, modes, img, 4, 4, pair)[inner]
                vals = set(np.unique(P).tolist())
                assert vals <= {2 * top, 2 * bot, top + bot} and top + bot in vals
                if pair != (0, 2):
                    assert vals == {2 * top, 2 * bot, top + bot}
                    edge = (P[:, :, :-1] != P[:, :, 1:]) & ((np.abs(P[:, :, :-1] - P[:, :, 1:])) >= 255 * q * M)
                    assert edge.any()
            K = R.stage_numerator(oh, modes, img, 4, 4)[inner]
            rim = 4 * cold
            assert (K.min() if not comp else K.max()) == rim and set(np.unique(K).tolist()) == {rim, rim + (hot - cold)}
            at = K[:, :, :-2] == rim
            assert (at & (K[:, :, 2:] != rim)).any() and ((K[:, :, :-1] == rim) & (K[:, :, 1:] != rim)).any()
            assert (R.stage_numerator(ch, modes, img, 4, 4)[inner] == 2 * (top + bot)).all()
    assert -128 * 4 * 16 * 4 == -32768 and 255 * 2 * 16 * 8 == 65280      # M = 4: the signed 16-bit rim of four rotations; M = 8: 65280 in a pair's unsigned field


# ---------------------------------------------------------------------------------------------
# two independent restatements agree on every table kind before a GPU is involved
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.TABLE_KINDS)
def test_host_emulators_give_the_oracles_bytes(emul, emul_iv, kind):  # noqa: F811
    for interval in (4, 5, 6):
        img = R.image(12, 64, 3, seed=interval, ragged=True)
        for final, u in ((False, 1), (True, 1), (True, 2), (True, 3), (True, 4)):
            for M in (1, 3, 4, 8):
                modes = R.SWEEP_LISTS[M]
                t = {m: R.table(kind, interval, u * u, ord(m), final) for m in set(modes)}
                luts = [t[m] for m in modes]
                want = c_oracle.stage(luts, modes, final, img, u, interval=interval)
                got = run_emul(emul, luts, modes, final, img, u) if interval == 4 else run_emul_iv(emul_iv, luts, modes, final, img, u, interval)
                assert np.array_equal(got, want), (interval, final, u, M)


def test_sweep_tables_too(emul, emul_iv):  # noqa: F811
    for (modes, interval, scale), draws in sorted(R.SWEEP_DRAWS.items()):
        if modes not in ("s", "sdys", "sdysdsd"):
            continue
        final, u, draw = scale > 0, max(scale, 1), draws[0]
        luts, img = R.sweep_tables(modes, interval, u, final, draw), R.sweep_image(draw)[:16]
        want = c_oracle.stage(luts, modes, final, img, u, interval=interval)
        got = run_emul(emul, luts, modes, final, img, u) if interval == 4 else run_emul_iv(emul_iv, luts, modes, final, img, u, interval)
        assert np.array_equal(got, want), (modes, interval, scale)
