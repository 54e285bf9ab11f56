"""Later stages and epilogues on inputs that reach their whole range (-m gpu).  Tables, images and draws come from tests/reach_cases.py;
tests/test_reach_cpu.py asserts, on the oracle alone, what they reach (every key level at every stage, both sides of the tube, every
rounding tie of every epilogue with both neighbours, opposite extremes in adjacent fields).  Here every route of every stage is held to
the oracle's bytes on them -- to the host emulators' for lists with e, h, o.  Bar: bit-exact."""
import numpy as np
import pytest

import reach_cases as R
from oracle import c_oracle
from test_core_math_cpu import emul, run_emul  # noqa: F401  (host emulator of mulut_core.h)
from test_interval_cpu import emul_iv, run_emul_iv  # noqa: F401  (host emulator of mulut_interval.h)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402

IV_LDS_BUDGET = 96 * 1024
ROW_BYTES = {1: 1, 2: 4, 3: 12, 4: 16}        # u x u int8 values, padded to whole dwords


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def check_forms(e, stage, img, want, tag):
    """One stage in every store form: HWC (packed RGB at x4), planar (dwords), two channels (byte-wise), planar in -> HWC out (what the
    final stage of a cascade runs: the only form the anchor-slab path takes)."""
    x, xp = dev(img), dev(img.transpose(2, 0, 1))
    assert np.array_equal(e.stage(stage, x).cpu().numpy(), want), tag + ("HWC",)
    assert np.array_equal(e.stage(stage, xp, layout=LAYOUT_CHW).cpu().numpy(), want.transpose(2, 0, 1)), tag + ("planar",)
    assert np.array_equal(e.stage(stage, dev(img[..., :2])).cpu().numpy(), want[..., :2]), tag + ("C=2",)
    assert np.array_equal(e.stage(stage, xp, layout=LAYOUT_CHW, out_layout=LAYOUT_HWC).cpu().numpy(), want), tag + ("planar->HWC",)


def one_byte_routes(e, final):
    """Every route of a stage with 1-byte rows at interval 4: routed, tube kernel on every tile, window kernel on every tile."""
    for first, name in ((0, "stage_u1t_kernel (smooth tiles) + stage_u1w_kernel (detailed tiles) + stage_u1_fix_kernel"),
                        (3, "stage_u1t_kernel + stage_u1_fix_kernel"), (2, "stage_u1w_kernel")):
        e.set_tuning("first_stage_kernel", first)
        assert e.kernel_name(final) == name, (first, e.kernel_name(final))
        yield ("first_stage_kernel", first)
    e.set_tuning("first_stage_kernel", 0)


def final_routes(e, scale, M):
    """Every route of a final stage at interval 4 (plan_stage): the name says which kernels run."""
    if scale == 1:
        yield from one_byte_routes(e, True)
        return
    if scale in (2, 3):
        tube = "stage_u1t_kernel<%d> + stage_up_fix_site_kernel<%d>" % (scale, scale)
        for sel in (0, 5, 1):
            e.set_tuning("final_stage_kernel", sel)
            assert e.kernel_name(True) == (tube if sel != 1 else "stage_up_kernel<generic>"), (sel, e.kernel_name(True))
            if sel == 0:        # the routed launch at its extremes: every tile left to the gather kernel, every tile kept
                for thr in (0, 1024, 8):
                    e.set_tuning("final_stage_detail_per_1024", thr)
                    yield ("final_stage_kernel", sel, "final_stage_detail_per_1024", thr)
            else:
                yield ("final_stage_kernel", sel)
        e.set_tuning("final_stage_kernel", 0)
        return
    for pipelined in (1, 0):
        e.set_tuning("tube_pipelined", pipelined)
        for detail in (0, 1):
            e.set_tuning("detail_kernel", detail)
            for sel, thr in ((0, 128), (1, 128), (5, 128), (6, 0), (6, 1024)):      # 128 is the threshold's default: selector 0 is the default mix
                e.set_tuning("final_stage_kernel", sel).set_tuning("hybrid_oob_per_1024", thr)
                name = e.kernel_name(True)
                lds = M <= 3 or (pipelined and M >= 3)          # lists of more than three modes run on stage_tube2_kernel or on the gather kernel
                if sel == 1 or not lds:
                    assert name.startswith("stage_up_kernel<4"), (M, pipelined, sel, name)
                else:
                    assert name.startswith("stage_tube" if sel == 5 else "hybrid: tile_stat_kernel + stage_tube"), (M, pipelined, sel, name)
                    if M >= 5:
                        assert "stage_tube2_kernel" in name and (sel == 5 or "stage_up_kernel<4,generic,wide> (detailed tiles)" in name), name
                    if not pipelined:
                        assert "stage_tube_kernel" in name, name
                    if sel != 5 and M <= 3:
                        assert ("stage_slab_kernel" in name) == (detail == 0), (detail, name)
                yield ("tube_pipelined", pipelined, "detail_kernel", detail, "final_stage_kernel", sel, thr)
    e.set_tuning("tube_pipelined", 1).set_tuning("detail_kernel", 0).set_tuning("final_stage_kernel", 0).set_tuning("hybrid_oob_per_1024", 128)


def interval_name(interval, u, M):
    lds = M * R.levels(interval) ** 4 * ROW_BYTES[u] <= IV_LDS_BUDGET
    return "stage_interval_kernel<%d,%d,%s>" % (interval, u, "lds" if lds else "global")


def stage_engine(modes, scale, interval, final, tables):
    """A context whose stage 1 is the stage under test: the only stage of a one-stage cascade (final), or the first of two."""
    e = MuLUTEngine(0).configure(1 if final else 2, modes, scale if final else 1, interval)
    for m, t in tables.items():
        e.set_lut(1, m, t)
        if not final:
            e.set_lut(2, m, t)
    return e


# ---------------------------------------------------------------------------------------------
# the epilogue sweep: every tie of every epilogue, on every route and store form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", range(1, 9))
@pytest.mark.parametrize("interval", [4, 5, 6])
def test_sweep_non_final(interval, M):
    modes = R.SWEEP_LISTS[M]
    e = None
    for draw in R.SWEEP_DRAWS[(modes, interval, 0)]:
        tables = R.sweep_luts(modes, interval, 1, False, draw)
        img = R.sweep_image(draw)
        want = c_oracle.stage([tables[m] for m in modes], modes, False, img, 1, interval=interval)
        if e is None:
            e = stage_engine(modes, 1, interval, False, tables)
        else:
            for m, t in tables.items():
                e.set_lut(1, m, t)
        if interval == 4:
            for route in one_byte_routes(e, False):
                check_forms(e, 1, img, want, (M, draw) + route)
        else:
            assert e.kernel_name(False) == "stage_interval_kernel<%d,1,lds>" % interval
            check_forms(e, 1, img, want, (M, draw))
    e.close()


@pytest.mark.parametrize("M", range(1, 9))
@pytest.mark.parametrize("interval,scale", [(4, 4), (4, 3), (4, 2), (4, 1), (5, 4), (5, 3), (5, 2), (5, 1), (6, 4), (6, 3), (6, 2), (6, 1)])
def test_sweep_final(interval, scale, M):
    """Every scale on its own draws, which reach every tie at that scale (test_reach_cpu.py).
    (The x1 final stage takes the integer epilogue; at interval 5 x2 the tables of up to three modes fit LDS and those of four and more
    are gathered from global memory, x4 is gathered for every list and interval 6 never leaves LDS.)"""
    modes = R.SWEEP_LISTS[M]
    e = None
    for draw in R.SWEEP_DRAWS[(modes, interval, scale)]:
        tables = R.sweep_luts(modes, interval, scale, True, draw)
        img = R.sweep_image(draw)
        want = c_oracle.stage([tables[m] for m in modes], modes, True, img, scale, interval=interval)
        if e is None:
            e = stage_engine(modes, scale, interval, True, tables)
        else:
            for m, t in tables.items():
                e.set_lut(1, m, t)
        if interval == 4:
            for route in final_routes(e, scale, M):
                check_forms(e, 1, img, want, (M, draw) + route)
        else:
            assert e.kernel_name(True) == interval_name(interval, scale, M)
            check_forms(e, 1, img, want, (M, draw))
    e.close()


@pytest.mark.parametrize("scale", [0, 4, 2])
@pytest.mark.parametrize("interval", [4, 5, 6])
@pytest.mark.parametrize("modes", R.WIDE_LISTS)
def test_sweep_wide_lists(emul, emul_iv, interval, modes, scale):  # noqa: F811
    """The wide kernels' epilogues on the wide lists' own draws, every one of them, whole: they reach every tie and both its neighbours
    (test_reach_cpu.py, on the NumPy restatement of the pass).  Against the host emulators; scale 0 is the non-final stage."""
    M, final, u = len(modes), scale > 0, max(scale, 1)
    e = None
    for draw in R.SWEEP_DRAWS[(modes, interval, scale)]:
        tables = R.sweep_luts(modes, interval, u, final, draw)
        img = R.sweep_image(draw)
        luts = [tables[m] for m in modes]
        want = run_emul(emul, luts, modes, final, img, u) if interval == 4 else run_emul_iv(emul_iv, luts, modes, final, img, u, interval)
        if e is None:
            e = stage_engine(modes, u, interval, final, tables)
        else:
            for m, t in tables.items():
                e.set_lut(1, m, t)
        if interval == 4:
            assert "wide" in e.kernel_name(final), e.kernel_name(final)
        else:
            assert e.kernel_name(final) == interval_name(interval, u, M)
        check_forms(e, 1, img, want, (modes, scale, draw))
    e.close()


# ---------------------------------------------------------------------------------------------
# checker and onehot tables (opposite extremes in adjacent fields) and ends tables, stage by stage on every route
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 4, 8])
@pytest.mark.parametrize("kind", ["checker", "checker_c", "onehot", "onehot_c", "ends"])
def test_table_kinds_on_every_route(kind, M):
    """M = 4 is the last list whose numerator fits the signed 16-bit field of stage_tube2_kernel's epilogue (onehot: K = -32768 at its
    rim), M = 8 fills the unsigned fields of a pair of rotations to 65280.  In the image's flat patches every pass reads single rows, so
    what one rotation adds up holds +127 q M beside -128 q M: in byte neighbours with checker, in dword halves with onehot
    (test_reach_cpu.py states this, and what the sums over two and four rotations hold, on the oracle)."""
    modes = R.SWEEP_LISTS[M]
    for ragged in (False, True):
        img = R.image(48, 128, 3, seed=M, ragged=ragged, flat=True)
        for final, scale in ((False, 1), (True, 4), (True, 3), (True, 2), (True, 1)):
            tables = {m: R.table(kind, 4, scale * scale, ord(m), final) for m in set(modes)}
            want = c_oracle.stage([tables[m] for m in modes], modes, final, img, scale)
            e = stage_engine(modes, scale, 4, final, tables)
            for route in (final_routes(e, scale, M) if final else one_byte_routes(e, False)):
                check_forms(e, 1, img, want, (kind, M, ragged, final, scale) + route)
            e.close()


@pytest.mark.parametrize("interval", [5, 6])
@pytest.mark.parametrize("kind", ["checker", "checker_c", "onehot", "onehot_c", "ends"])
def test_table_kinds_at_intervals_5_and_6(kind, interval):
    img = R.image(48, 128, 3, seed=interval, ragged=True, flat=True)
    for M in (1, 3, 4, 8):
        modes = R.SWEEP_LISTS[M]
        for final, scale in ((False, 1), (True, 4), (True, 2)):
            tables = {m: R.table(kind, interval, scale * scale, ord(m), final) for m in set(modes)}
            want = c_oracle.stage([tables[m] for m in modes], modes, final, img, scale, interval=interval)
            e = stage_engine(modes, scale, interval, final, tables)
            assert e.kernel_name(final) == interval_name(interval, scale, M)
            check_forms(e, 1, img, want, (kind, interval, M, final, scale))
            e.close()


@pytest.mark.parametrize("modes", R.WIDE_LISTS)
@pytest.mark.parametrize("kind", ["checker", "checker_c", "onehot", "onehot_c", "ends"])
def test_table_kinds_on_wide_lists(emul, emul_iv, kind, modes):  # noqa: F811
    """The same tables on the wide kernels (merged rotation pairs) and on the interval kernels with wide lists, against the host emulators."""
    M = len(modes)
    for interval in (4, 5, 6):
        img = R.image(48, 128, 3, seed=interval + M, ragged=True, flat=True)
        for final, scale in ((False, 1), (True, 4), (True, 2)):
            tables = {m: R.table(kind, interval, scale * scale, ord(m), final) for m in set(modes)}
            luts = [tables[m] for m in modes]
            want = run_emul(emul, luts, modes, final, img, scale) if interval == 4 else run_emul_iv(emul_iv, luts, modes, final, img, scale, interval)
            e = stage_engine(modes, scale, interval, final, tables)
            if interval == 4:
                assert "wide" in e.kernel_name(final), e.kernel_name(final)
            else:
                assert e.kernel_name(final) == interval_name(interval, scale, M)
            check_forms(e, 1, img, want, (kind, modes, interval, final, scale))
            e.close()


# ---------------------------------------------------------------------------------------------
# cascades whose every stage sees every level
# ---------------------------------------------------------------------------------------------
def cascade_want(emul_lib, luts, case, img):
    stages, scale, modes, interval = case
    if not set(modes) & set("eho"):
        return c_oracle.pipeline(luts, stages, modes, scale, img, interval=interval)
    cur = img
    for s in range(stages):
        last = s + 1 == stages
        cur = run_emul(emul_lib, [luts["s%d_%s" % (s + 1, m)] for m in modes], modes, last, cur, scale if last else 1)
    return cur


@pytest.mark.parametrize("kind", ["ramp", "ends", "checker", "checker_c", "onehot", "onehot_c"])
@pytest.mark.parametrize("case", R.CASCADES, ids=lambda c: "%dx%d-%s-iv%d" % c)
def test_cascades(emul, case, kind):  # noqa: F811
    stages, scale, modes, interval = case
    luts = R.cascade_luts(kind, stages, modes, scale, interval)
    e = MuLUTEngine(0).configure(stages, modes, scale, interval).set_lut_dict(luts)
    for ragged in (False, True):
        img = R.cascade_image(case, ragged)
        h = img.shape[0]
        want = cascade_want(emul, luts, case, img)
        sels = (0, 5, 1) if interval == 4 and not set(modes) & set("eho") else (0,)
        for sel in sels:
            e.set_tuning("final_stage_kernel", sel)
            assert np.array_equal(e.pipeline(dev(img)).cpu().numpy(), want), (case, kind, ragged, sel)
        e.set_tuning("final_stage_kernel", 0)
        got = e.pipeline(dev(img.transpose(2, 0, 1)), layout=LAYOUT_CHW).cpu().numpy()
        assert np.array_equal(got.transpose(1, 2, 0), want), (case, kind, ragged, "planar")
        mid, halo = h // 2, e.halo                           # two strips
        top = e.pipeline_rows(dev(img[: mid + halo]), 0, 0, mid, h)
        bot = e.pipeline_rows(dev(img[mid - halo:]), mid - halo, mid, h, h)
        assert np.array_equal(torch.cat([top, bot], 0).cpu().numpy(), want), (case, kind, ragged, "strips")
    e.close()


@pytest.mark.parametrize("kind", ["ramp", "ends"])
def test_detailed_tiles_span_the_sixteen_slab_pairs(kind):
    """The final stage's noisy half holds every anchor MSB (test_reach_cpu.py), so every slab pair A = 0 .. 15 runs samples; the counters
    only show that the slab path ran -- the bytes are the oracle's, the gather kernel's, and the same twice."""
    luts = R.cascade_luts(kind, 2, "sdy", 4, 4)
    img = R.image(seed=6)
    want = c_oracle.pipeline(luts, 2, "sdy", 4, img)
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(luts)
    assert "stage_slab_kernel" in e.kernel_name(True)
    got = e.pipeline(dev(img))
    cnt = e.last_detail_counters()
    assert np.array_equal(got.cpu().numpy(), want)
    assert len(cnt["samples_per_anchor"]) == 16 and min(cnt["samples_per_anchor"]) > 0 and cnt["items"] > 0, cnt
    assert torch.equal(e.pipeline(dev(img)), got)
    e.set_tuning("detail_kernel", 1)
    assert "stage_slab_kernel" not in e.kernel_name(True)
    assert torch.equal(e.pipeline(dev(img)), got)
    e.close()


def test_ramp_cascade_replays_from_a_captured_graph():
    case = (2, 4, "sdy", 4)
    luts = R.cascade_luts("ramp", 2, "sdy", 4, 4)
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(luts)
    img = np.stack([R.cascade_image(case), R.image(seed=9)])
    n, h, w, c = img.shape
    x = dev(img)
    out = torch.empty((n, 4 * h, 4 * w, c), dtype=torch.uint8, device="cuda")
    e.reserve(n, h, w, c)                         # no allocation inside the captured region
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        e.pipeline(x, out=out)                    # warm-up: kernel attributes are set on first launch
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e.pipeline(x, out=out)
    for trial in range(2):
        cur = np.roll(img, 7 * trial, axis=2)
        x.copy_(dev(cur))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), np.stack([c_oracle.pipeline(luts, 2, "sdy", 4, im) for im in cur])), trial
    e.close()
