"""The premises of tests/test_gpu_ft_abi.py, checked without a GPU:
  * the case list reaches every kernel instance and form of the fine-tune half (launch rules restated in tests/ft_abi_cases.py), the
    cases built for the memory fallback of the input-gradient tile really exceed it, and no shape is larger than 16 x 1 x 48 x 48;
  * every case's reference is integral and under the exactness cap -- also prefilled and run twice (the accumulate test);
  * the arena harness lays buffers out as it says;
  * ft_pass_setup() of mulut_amd/csrc/mulut_ft.h, compiled by g++ (tests/host_emul/emul_ft_clamp.cpp): inside the table and the
    tube band for every key value, and equal to the set-up without the clamp wherever the ABI's precondition holds;
  * the module's stage function checks its arguments before it loads the library."""
import ctypes

import numpy as np
import pytest
import torch

import ft_abi_cases as fa
import ft_exact_cases as fx
from host_emul_lib import load_emul

PATTERNS = {"s": ((0, 1), (1, 0), (1, 1)), "d": ((0, 2), (2, 0), (2, 2)), "y": ((1, 1), (1, 2), (2, 1)),
            "e": ((0, 3), (3, 0), (3, 3)), "h": ((2, 2), (2, 3), (3, 2)), "o": ((2, 2), (1, 3), (3, 1))}


# ---------------------------------------------------------------------------------------------------------------- the case list
def test_case_list_reaches_every_kernel_instance_and_form():
    reached = set()
    for c in fa.CASES:
        reached |= fa.reach_of(c)
    missing = fa.required_reach() - reached
    assert not missing, sorted(missing)
    for c in fa.CASES + fa.EXTRA:
        assert int(np.prod(c.shape)) <= fa.LARGEST, c.name
    # every interval runs through each of its entry-point families, the wide lists through the wide one
    fams = {(c.interval, e) for c in fa.CASES for e in fa.entries_of(c)}
    assert fams == {(4, "plain"), (4, "mask"), (4, "wide"), (5, "interval"), (5, "wide"), (6, "interval"), (6, "wide")}
    assert {c.interval for c in fa.CASES if fa.is_wide(c)} == {4, 5, 6}


def test_wide_cases_exceed_the_input_gradient_tile_and_small_ones_fit():
    for c in fa.CASES:
        if c.u == 4:
            continue
        fits = fa.wave_tiles_fit(c)
        if c.shape in ((1, 2, 3, 300), (1, 1, 4, 260)):
            assert not any(fits), (c.name, fits)
            B, C, H, W = c.shape
            assert (H + 2 * fa.halo_of(c)) * (W + 2 * fa.halo_of(c)) > fa.GX_TILE
        elif c.shape in ((2, 1, 13, 10), (1, 2, 9, 11), (1, 1, 1, 7)):
            assert all(fits), (c.name, fits)
    # tiles that straddle a plane boundary: a wave of (1, 2, 9, 11) holds sites of both planes
    assert 9 * 11 % 64 != 0 and 9 * 11 < 2 * 64


@pytest.mark.parametrize("case", fa.CASES + fa.EXTRA, ids=lambda c: c.name)
def test_reference_is_exact_also_prefilled_and_run_twice(case):
    case, ref = fa.built(case)       # asserts integrality, the cap of one call and the case's reach on the oracle alone
    cap2 = fa.accumulate_cap(case, ref, calls=2)
    print(case.name, "one call: sum |terms| * q =", ref.cap, " grad_x bound =", fa.gx_bound(case), " prefilled, two calls:", cap2)
    assert cap2 < fa.CAP, (case.name, cap2)
    assert int(np.abs(ref.gx_num).max()) <= fa.gx_bound(case)
    pw, px = fa.prefill(case)
    assert all(int(np.abs(p).max()) <= fa.PREFILL for p in pw + [px])
    for m in range(case.M):      # prefilled elements the case does not touch, and touched ones: both exist (except the one-pixel image)
        touched = ref.gw_num[m] != 0
        assert (pw[m][~touched] != 0).any() or touched.mean() > 0.9      # (a dense case on the 625 rows of interval 6 touches them all)
        if case.shape != (1, 1, 1, 1):
            assert touched.any() and (pw[m][touched] != 0).any()
        fa.as_f32(pw[m] + 2 * ref.gw_num[m], case.q)
    fa.as_f32(px + 2 * ref.gx_num, case.q)


def test_stream_and_capture_cases_stay_exact_through_the_quantiser_backward():
    """grad * 127 after the stage backward: 127 * sum |terms| * q must stay under the cap as well"""
    for key, first in fa.FAMILY_CASES.items():
        second = fa.SECOND[key]
        assert first.shape == second.shape and first.modes == second.modes and first.name != second.name
        assert (first.interval, first.u, first.last) == (second.interval, second.u, second.last)
        assert fa.FAMILY_ENTRY[key] in fa.entries_of(first)
        for c in (first, second):
            case, ref = fa.built(c)
            assert 127 * ref.cap < fa.CAP, (c.name, ref.cap)
        assert not np.array_equal(fa.built(first)[0].x, fa.built(second)[0].x)


# --------------------------------------------------------------------------------------------------------------------- the arena
def test_arena_layout_offsets_slack_and_checks():
    case = fx.Case(4, 2, 1, "sd", (1, 1, 3, 5), "noise")
    for k in fa.OFFSETS:
        for backward in (False, True):
            a = fa.stage_arena(case, k, backward, True)
            spans = sorted((off, off + n, name) for name, (off, n, _) in a.items.items())
            assert spans[0][0] >= fa.SLACK and a.size - spans[-1][1] >= fa.SLACK
            for (_, hi, _), (lo, _, _) in zip(spans, spans[1:]):
                assert lo - hi >= 2 * fa.SLACK            # a slack of its own on either side
            for name, (off, n, kind) in a.items.items():
                assert (off % 4 == 2) if name == "inside" else (off % 16 == k), (name, off)
            contents = {name: np.zeros(n, np.uint8) for name, (off, n, kind) in a.items.items()}
            img = a.image(contents)
            for name, (off, n, kind) in a.items.items():
                if kind == "in":          # NaN on the buffer's own float grid, on both sides
                    assert np.isnan(img[off - 64:off].view(np.float32)).all()
                    assert np.isnan(img[off + n:off + n + 64].view(np.float32)).all()
                else:
                    assert (img[off - fa.SLACK:off] == (fa.FILL if kind == "out" else 0xFF)).all()
            assert a.outside_changed(img, img.copy(), ()) == []
            hit = img.copy()
            off, n, _ = a.items["x"]
            hit[off - 1] ^= 1
            assert any("slack of x" in b for b in a.outside_changed(img, hit, ()))
            hit = img.copy()
            hit[off] ^= 1
            assert a.outside_changed(img, hit, ()) == ["x is an input and was changed"]


# --------------------------------------------------------------------------------------------------------------------- the clamp
@pytest.fixture(scope="module")
def emul():
    L = load_emul("emul_ft_clamp", ["mulut_core.h", "mulut_ft.h"], ["-ffp-contract=off"])
    L.emul_ft4_passes.restype = None
    L.emul_ft4_passes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5
    return L


def passes(L, plane, mode, clamped):
    plane = np.ascontiguousarray(plane, np.float32)
    H, W = plane.shape
    di = np.array([o[0] for o in PATTERNS[mode]], np.int32)
    dj = np.array([o[1] for o in PATTERNS[mode]], np.int32)
    n = H * W * 4
    idx, wt, ts = np.zeros((n, 5), np.int32), np.zeros((n, 5), np.float32), np.zeros((n, 5), np.int32)
    tube, ord_ = np.zeros(n, np.int32), np.zeros(n, np.int32)
    L.emul_ft4_passes(plane.ctypes.data, H, W, di.ctypes.data, dj.ctypes.data, int(clamped), idx.ctypes.data, wt.ctypes.data, ts.ctypes.data,
                      tube.ctypes.data, ord_.ctypes.data)
    return idx, wt, ts, tube, ord_


def test_clamped_setup_stays_inside_the_table_and_the_tube_for_any_key_value(emul):
    """x in {-300, -1, -0.5, 255.5, 256, 1e9, +-inf, NaN} at each of the four key positions and every rotation (a bad pixel in the
    middle of a 7 x 7 plane is key a of its own site and key b, c or d of the sites around it, under every rotation; borders come
    from planes of one value), all six patterns: every row in [0, 83521), every tube slot in [0, 1041)."""
    rows, slots = emul.emul_ft4_rows(), emul.emul_ft4_tube_slots()
    assert (rows, slots) == (83521, 1041)
    rng = np.random.default_rng(7)
    for v in fa.BAD_VALUES + (300.0, -1e9, 1e30, -1e30, 4e9, 255.99):
        for mode in PATTERNS:
            reach = max(max(o) for o in PATTERNS[mode])
            base = rng.integers(0, 256, (7, 7)).astype(np.float32)
            one = base.copy()
            one[3, 3] = v
            for plane in (one, np.full((7, 7), v, np.float32), np.where(rng.random((7, 7)) < 0.5, np.float32(v), base)):
                idx, wt, ts, tube, _ = passes(emul, plane, mode, True)
                assert idx.min() >= 0 and idx.max() < rows, (v, mode, int(idx.min()), int(idx.max()))
                assert ts.min() >= 0 and ts.max() < slots, (v, mode, int(ts.min()), int(ts.max()))
            # the single bad pixel is read as each key under each rotation
            bad_site = ~np.isfinite(passes(emul, one, mode, True)[1]).all(-1) if not np.isfinite(v) else None
            if bad_site is not None:
                per_rot = bad_site.reshape(7, 7, 4)
                assert per_rot[3, 3].all() and all(per_rot[:, :, r].sum() == 4 for r in range(4)), (v, mode, reach)


def test_clamped_setup_is_a_permutation_inside_the_table_for_every_mix_of_bad_keys(emul):
    """Every quadruple over a pool of key values -- NaN of both signs, negative denormals (their quotient by q underflows to -0 and the
    LSB keeps the sign bit), -0, infinities, values the int conversion cannot hold, and in-range values at MSB 0 and 15 -- as keys
    a, b, c, d of ONE pass.  With a sign-set LSB ranked as it stands the six comparisons of ft_order_code() form cycles (anchor 255
    with -NaN, +NaN, 0 gave row 83539; with -2^-149, 0, 8 row 83811): the set-up ranks |LSB|, so the code is a permutation of the
    four keys for every quadruple, every row lies in [0, 83521) and every tube slot in [0, 1041).  The MSB is clamped in float, so
    the conversion is defined: +inf and 1e30 sit at MSB 15, NaN and -inf at 0, here as on the device."""
    pool = np.array([fa.NEG_NAN, np.nan, fa.NEG_DENORMAL, fa.f32_bits(0x80000008), fa.f32_bits(0x807FFFFF), -0.0, fa.f32_bits(1), np.inf, -np.inf,
                     1e30, -1e30, 4e9, 1e9, -300.0, -1.0, -0.5, 255.5, 256.0, 300.0, 255.0, 247.5, 240.0, 8.0, 0.0, 15.0, 16.0], np.float32)
    assert np.signbit(pool[0]) and np.isnan(pool[0]) and not np.signbit(pool[1]) and pool[2] < 0 and pool[2] / np.float32(16) == 0
    n = len(pool)
    g = np.stack(np.meshgrid(*[np.arange(n)] * 4, indexing="ij"), -1).reshape(-1, 4)
    quads = np.ascontiguousarray(pool[g])
    idx, ts, ord_ = np.zeros((len(quads), 5), np.int32), np.zeros((len(quads), 5), np.int32), np.zeros(len(quads), np.int32)
    emul.emul_ft4_quads.restype = None
    emul.emul_ft4_quads.argtypes = [ctypes.c_void_p, ctypes.c_long] + [ctypes.c_void_p] * 3
    emul.emul_ft4_quads(quads.ctypes.data, len(quads), idx.ctypes.data, ts.ctypes.data, ord_.ctypes.data)
    keys = np.stack([(ord_ >> (2 * j)) & 3 for j in range(4)], -1)
    not_perm = np.sort(keys, -1) != np.arange(4)
    assert not not_perm.any(), quads[not_perm.any(-1)][:4]
    assert idx.min() >= 0 and idx.max() <= 83520, (int(idx.min()), int(idx.max()), quads[(idx > 83520).any(-1)][:4])
    assert ts.min() >= 0 and ts.max() <= 1040, (int(ts.min()), int(ts.max()), quads[(ts > 1040).any(-1)][:4])
    assert np.array_equal(idx[:, 4], idx[:, 0] + 5220) and np.array_equal(ts[:, 4], ts[:, 0] + 65)
    # the reviewer-style cases by name, and the MSBs of the values no int holds
    def first_row(a, b, c, d):
        hit = np.flatnonzero((quads.view(np.uint32) == np.array([a, b, c, d], np.float32).view(np.uint32)).all(-1))
        return idx[hit[0]]
    assert first_row(255.0, fa.NEG_NAN, np.nan, 0.0)[0] == 15 * 4913 and first_row(255.0, fa.NEG_DENORMAL, 0.0, 8.0)[4] == 15 * 4913 + 5220
    assert first_row(np.inf, np.inf, 1e30, 4e9)[0] == 15 * 5220 and first_row(np.nan, fa.NEG_NAN, -np.inf, -1e30)[0] == 0


def test_clamped_setup_equals_the_unclamped_one_on_every_allowed_key_value(emul):
    """all integer and half-integer x in 0..255 (every MSB / LSB pair, ties included): rows, weights (bit for bit), tube slots, the
    in-tube flag and the order code are what the set-up without the clamp computes"""
    vals = np.arange(0, 511, dtype=np.float32) / 2        # 0, 0.5, ..., 255
    assert vals[-1] == 255 and len(vals) == 511
    rng = np.random.default_rng(11)
    planes = [vals[rng.integers(0, len(vals), (24, 24))] for _ in range(4)]
    planes.append(np.resize(vals, (24, 24)))              # every value, neighbours half a level apart
    planes.append(rng.choice(np.array([0, 15, 15.5, 16, 239.5, 240, 255], np.float32), (24, 24)))      # both rims, ties
    seen = set()
    for plane in planes:
        seen |= set(np.unique(plane).tolist())
        for mode in PATTERNS:
            got, want = passes(emul, plane, mode, True), passes(emul, plane, mode, False)
            for g, w, what in zip(got, want, ("rows", "weights", "tube slots", "in_tube", "order")):
                assert np.array_equal(g.view(np.int32), w.view(np.int32)), (mode, what)
            assert got[0].max() <= 83520 and (got[1] >= 0).all() and np.array_equal(got[1].sum(-1), np.full(len(got[1]), 16, np.float32))
    assert seen == set(vals.tolist())


def test_poisoned_cases_leave_sites_to_compare_and_hit_corners():
    for case in fa.CLAMP_CASES:
        case, _ = fa.built(case)
        x, hit, changed = fa.poisoned(case)
        assert int(changed.sum()) == len(fa.BAD_VALUES) + 16 and np.isinf(x).sum() == 2 and np.isnan(x).sum() == 1 + 4
        assert int((np.isnan(x) & np.signbit(x)).sum()) == 2 and int(((x < 0) & (x > -1e-40)).sum()) == 2      # -NaN and negative denormals
        assert changed[0, 0, 0, 0] and changed[-1, -1, -1, -1] and (hit | ~changed).all()
        assert 0.3 < (~hit).mean() < 0.9, (~hit).mean()          # enough sites on either side
        assert np.array_equal(x[~changed], case.x[~changed])
        # under pattern s, rotation 0, a pass of the block reads 255, -NaN, NaN, 0 -- the anchor at MSB 15 next to a sign-set LSB
        assert fa.BAD_BLOCK[0, 0] == 255 and np.signbit(fa.BAD_BLOCK[0, 1]) and np.isnan(fa.BAD_BLOCK[1, 0]) and fa.BAD_BLOCK[1, 1] == 0


# -------------------------------------------------------------------------------------------------------------------- the module
def test_stage_function_refuses_a_host_tensor_before_the_library_is_loaded(monkeypatch):
    """the refusals of _StageFn.forward precede any library call: with the loader made to fail, a host x still gets the TypeError.
    (That a CUDA x of another dtype is refused is held on the GPU: test_gpu_ft_abi.py.)"""
    from mulut_amd import _native
    from mulut_amd.finetune import _StageFn

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_native, "load", no_load)
    w = torch.zeros((83521, 1), dtype=torch.float32)
    with pytest.raises(TypeError):
        _StageFn.apply(torch.zeros((1, 1, 4, 4), dtype=torch.float32), "s", False, 1, 4, w)


# ------------------------------------------------------------------------------------------------------------ the shared case objects
def test_built_cases_outlive_the_tests_that_release_the_shared_objects():
    """The objects of fa.CASES are those of ft_exact_cases.CASES / ft_wide_cases.CASES (_pick returns them).  The tests that own those
    lists (test_ft_exact_cpu.py, test_ft_wide_cpu.py, test_gpu_ft_exact.py, test_gpu_ft_wide.py) build a case and release its arrays
    per test, and tests/test_gpu_abi_streams.py ran the same path on them.  In one process with them, before or after, built() must
    still hand out a case with its arrays: it holds a copy, and the stream test builds on a copy of its own."""
    import test_gpu_abi_streams as streams      # (importing it needs no GPU: every collection does)
    shared = [c for c in streams.FT_CASES if any(c is d for d in fa.CASES)]
    assert len(shared) >= 6 and {c.interval for c in shared} == {4, 5, 6}
    for k, case in enumerate(shared):
        if k % 2:
            fa.built(case)
        before = dict(vars(case))
        ref, tables, x, gout = streams._reference_and_inputs(case, lambda a: a)
        assert vars(case) == before      # the stream test's path leaves the object it was given alone
        assert len(tables) == case.M and x.shape == case.shape and gout.dtype == np.float32 and ref.out is not None
        case.build()                     # what an owner's test does with it
        case.tables = case.x = case.gout = None
        got, _ = fa.built(case)
        assert got is not case and got.name == case.name and got.tables is not None and got.x is not None and got.gout is not None
        assert np.array_equal(got.x, x) and np.array_equal(got.gout, gout) and all(np.array_equal(a, b) for a, b in zip(got.tables, tables))
