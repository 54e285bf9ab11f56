"""One context through a long life (-m gpu): the operation sequences of tests/abi_sequences.py against their model after every call,
and the state hazards include/mulut.h names or the code implies -- first-stage tile marks that outlive the content they were made
for, a captured graph after a table rewrite, the timing state across a reconfiguration, caller buffers at odd addresses.
Expected bytes come from the C oracle / the host emulators (abi_sequences.ref_*), never from the library."""
import re

import numpy as np
import pytest

import abi_sequences as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine, MuLUTError  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402
from oracle import c_oracle  # noqa: E402

assert (LAYOUT_CHW, LAYOUT_HWC) == (A.CHW, A.HWC)


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def to_layout(nhwc, layout):
    return nhwc if layout == LAYOUT_HWC else np.ascontiguousarray(nhwc.transpose(0, 3, 1, 2))


def from_layout(t, layout):
    a = t.cpu().numpy()
    return a if layout == LAYOUT_HWC else np.ascontiguousarray(a.transpose(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------------------------ sequences
def run_op(e, op, held):
    """Run one operation on the engine; returns what it gave in the form the model states it (bytes in NHWC / a count / None)."""
    a = op.args
    if op.name == "configure":
        e.configure(a["stages"], a["modes"], a["scale"], a["interval"])
    elif op.name == "set_lut":
        e.set_lut(a["stage"], a["mode"], a["table"])
    elif op.name == "set_tuning":
        e.set_tuning(a["key"], a["val"])
    elif op.name == "pipeline":
        return from_layout(e.pipeline(dev(to_layout(a["img"], a["layout"])), layout=a["layout"]), a["layout"])
    elif op.name == "pipeline_rows":
        out = e.pipeline_rows(dev(to_layout(a["band"], a["layout"])), a["band_row0"], a["y0"], a["y1"], a["H_full"], layout=a["layout"])
        return from_layout(out, a["layout"])
    elif op.name == "stage":
        x = held["prev"] if a["from_prev"] else dev(to_layout(a["img"], a["layout"]))     # from_prev: the very buffer the stage before wrote
        out = e.stage(a["stage"], x, layout=a["layout"], out_layout=a["out_layout"])
        held["prev"] = out if a["out_layout"] == LAYOUT_CHW else None
        return from_layout(out, a["out_layout"])
    elif op.name == "pass_q":
        return e.pass_q(a["stage"], a["mode"], a["r"], dev(a["img"])).cpu().numpy()
    elif op.name == "reserve":
        e.reserve(a["N"], a["H"], a["W"], a["C"])
    elif op.name == "set_stage_timing":
        e.set_stage_timing(a["enable"])
    elif op.name == "last_stage_ms":
        ms = e.last_stage_ms()
        assert all(v > 0 for v in ms), ms
        return len(ms)
    elif op.name == "last_kernel_ms":
        return len(e.last_kernel_ms())
    elif op.name == "last_detail_counters":
        c = e.last_detail_counters()
        assert set(c) >= {"samples_per_anchor", "items", "fix_pixels"}
    else:
        raise AssertionError("unknown operation " + op.name)
    return None


def outcome(e, op, held):
    try:
        got = run_op(e, op, held)
    except MuLUTError as ex:
        return "error", int(re.match(r"mulut error (-?\d+)", str(ex)).group(1))
    except ValueError as ex:                # the binding raises the reference's ValueError for MULUT_EMODE
        assert "Mode not implemented" in str(ex), ex
        return "error", A.EMODE
    return ("bytes" if isinstance(got, np.ndarray) else "count" if isinstance(got, int) else "ok"), got


@pytest.mark.parametrize("k", range(A.CONTEXTS))
def test_sequence_matches_the_model_after_every_call(k):
    ops = A.sequences()[k]
    e = MuLUTEngine(0)
    held = {"prev": None}
    for i, op in enumerate(ops):
        kind, got = outcome(e, op, held)
        where = "sequence %d, operation %d; the last three:\n  %s" % (k, i, "\n  ".join(o.brief() for o in ops[max(0, i - 2):i + 1]))
        assert kind == op.kind, "%s\ngot %s %r" % (where, kind, got if kind != "bytes" else got.shape)
        if kind == "bytes":
            assert got.shape == op.value.shape and np.array_equal(got, op.value), "%s\n%d of %d bytes differ" % (
                where, int((got != op.value).sum()) if got.shape == op.value.shape else -1, op.value.size)
        elif kind in ("error", "count"):
            assert got == op.value, "%s\ngot %s %r" % (where, kind, got)
    e.close()


# ------------------------------------------------------------------------------------------------------------------ stale marks
def _marks_case(shipped_luts):
    H, W = 256, 320                 # 4 x 5 tiles of 64 x 64
    smooth = natural_frames(1, H, W, 3, seed=5)[0]
    noise = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    l1, l2 = [shipped_luts["s1_" + m] for m in "sdy"], [shipped_luts["s2_" + m] for m in "sdy"]
    mid = c_oracle.stage(l1, "sdy", False, noise, 1)            # what a first stage writes for the noise frame (from the oracle:
    return smooth, mid, l2                                      # the engine's own marks stay those of the smooth frame)


@pytest.mark.parametrize("variant", ["overwritten", "reallocated", "channels"])
def test_final_stage_is_exact_on_marks_made_for_other_content(shipped_luts, variant):
    """mulut_stage(1, x -> A) leaves per-tile marks keyed on A's address and shape; the next final-stage launch that reads that
    address trusts them.  Here A holds OTHER content by then: overwritten in place, a new tensor the allocator put at the same
    address (skipped when it did not), or one plane of it (C = 3, then C = 1).  The marks were made for a smooth frame (nothing
    marked), the content is the first-stage output of a noise frame (every tile detailed): the statistic sends every tile to the
    tube kernel where the stale marks say "smooth", and its out-of-band samples go through the fix-up list -- more fix-up work,
    the same bytes.  The counters of the two settings show that the marks were consumed.
    Observed on the MI355X (256 x 320 frames; stat_from_first_stage 1 / 0): overwritten and reallocated, C = 3: 14,208 / 2,048
    fix-up entries, 227,712 / 239,616 samples on the slab path in 230 / 242 work items; one plane, C = 1: 6,016 / 2,048 entries,
    75,904 / 79,872 samples in 82 / 87 items.  (The first stage had marked most tiles of the photograph-like frame itself, so most
    tiles were still looked at; the ones it had left unmarked went to the tube kernel unseen.)  Exact in every case.  The
    reallocated variant runs whenever torch's caching allocator hands the released block back for the same size, which it does
    after empty_cache() (then that block is its only free one of the size); it skips only if the addresses differ."""
    smooth, mid, l2 = _marks_case(shipped_luts)
    C = 1 if variant == "channels" else 3
    content = np.ascontiguousarray(mid[:, :, :C].transpose(2, 0, 1))
    want = c_oracle.stage(l2, "sdy", True, mid[:, :, :C], 4).transpose(2, 0, 1)
    counters = {}
    for stat in (1, 0):
        e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(shipped_luts)
        e.set_tuning("stat_from_first_stage", stat)
        if variant == "reallocated":
            torch.cuda.synchronize()
            torch.cuda.empty_cache()        # no other free block of this size: the released address is the allocator's best fit
        x0 = dev(smooth.transpose(2, 0, 1))
        a = e.stage(1, x0, layout=LAYOUT_CHW, out_layout=LAYOUT_CHW)
        if variant == "reallocated":
            ptr, shape = a.data_ptr(), a.shape
            torch.cuda.synchronize()
            del a
            a = torch.empty(shape, dtype=torch.uint8, device="cuda")
            if a.data_ptr() != ptr:
                pytest.skip("the caching allocator did not hand the released address to the new tensor")
            assert a.data_ptr() == ptr
            a.copy_(torch.from_numpy(content))
            x = a
        elif variant == "channels":
            a[0].copy_(torch.from_numpy(content[0]))
            x = a[:1]
            assert x.data_ptr() == a.data_ptr() and x.is_contiguous()
        else:
            a.copy_(torch.from_numpy(content))
            x = a
        got = e.stage(2, x, layout=LAYOUT_CHW, out_layout=LAYOUT_CHW).cpu().numpy()
        counters[stat] = e.last_detail_counters()
        print(variant, "stat_from_first_stage", stat, "items", counters[stat]["items"], "fix entries", counters[stat]["fix_pixels"],
              "slab samples", sum(counters[stat]["samples_per_anchor"]))
        assert np.array_equal(got, want), (variant, stat, int((got != want).sum()))
        e.close()
    # the marks were consumed: tiles the statistic did not look at went to the tube kernel, whose misses are on the fix-up list
    assert counters[1]["fix_pixels"] > counters[0]["fix_pixels"], counters
    assert sum(counters[1]["samples_per_anchor"]) < sum(counters[0]["samples_per_anchor"]), counters


# ------------------------------------------------------------------------------------------------- graph after a table rewrite
@pytest.mark.parametrize("stages,modes,scale,interval", [(2, "sdy", 4, 4), (2, "sdy", 2, 4), (2, "sdyeho", 4, 4), (2, "sdy", 4, 6)])
def test_captured_graph_reads_a_table_rewritten_in_place(stages, modes, scale, interval):
    """mulut.h, hipGraph note: "setting a table of the same shape rewrites it in place, so a captured graph then reads the new
    values" -- the full table, and at interval 4 the tube band and the slab image derived from it.
    Only what the header calls valid is replayed: the graphs the header calls INVALID (after a larger call, a table of another
    size, an interval change) would read freed memory on a shared machine and are never replayed here."""
    rng = np.random.default_rng(stages + scale + interval)
    tables = {(s, m): A.make_table(rng, interval, scale * scale if s == stages else 1, True)
              for s in range(1, stages + 1) for m in dict.fromkeys(modes)}
    e = MuLUTEngine(0).configure(stages, modes, scale, interval)
    for (s, m), t in tables.items():
        e.set_lut(s, m, t)
    img = A.natural_noise(2, 40, 68, 3, seed=9)
    x = dev(img)
    out = torch.empty((2, 40 * scale, 68 * scale, 3), dtype=torch.uint8, device="cuda")
    e.reserve(2, 40, 68, 3)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        e.pipeline(x, out=out)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e.pipeline(x, out=out)

    def replay():
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        return out.cpu().numpy()

    want = np.stack([A.ref_pipeline(tables, stages, modes, scale, im, interval) for im in img])
    assert np.array_equal(replay(), want), "before the rewrite"
    for s in range(1, stages + 1):                  # one table of each stage: other rows, same shape
        m = modes[(s - 1) % len(modes)]
        tables[(s, m)] = A.make_table(rng, interval, tables[(s, m)].shape[1], s % 2 == 0)
        e.set_lut(s, m, tables[(s, m)])
    new = np.stack([A.ref_pipeline(tables, stages, modes, scale, im, interval) for im in img])
    assert not np.array_equal(new, want)
    assert np.array_equal(replay(), new), "after the rewrite"
    e.close()


# ---------------------------------------------------------------------------------------------------------------- timing state
def test_timing_state_follows_the_configuration_and_never_changes_results():
    rng = np.random.default_rng(1)
    img = A.natural_noise(1, 64, 128, 3, seed=2)
    e = MuLUTEngine(0)
    tables = {stages: {(s, m): A.make_table(rng, 4, 4 if s == stages else 1, True) for s in range(1, stages + 1) for m in "sdy"}
              for stages in (4, 2)}
    want = {stages: A.ref_pipeline(tables[stages], stages, "sdy", 2, img[0], 4) for stages in (4, 2)}

    def setup(stages):
        e.configure(stages, "sdy", 2, 4)
        for (s, m), t in tables[stages].items():
            e.set_lut(s, m, t)

    for stages in (4, 2):
        setup(stages)
        plain = e.pipeline(dev(img)).cpu().numpy()
        assert e.last_stage_ms() == [] and e.last_kernel_ms() == []         # off: nothing
        e.set_stage_timing(True)
        timed = e.pipeline(dev(img)).cpu().numpy()
        ms, kms = e.last_stage_ms(), e.last_kernel_ms()
        assert len(ms) == stages and all(v > 0 for v in ms), (stages, ms)
        assert len(kms) == stages and all(k > 0 for k in kms), (stages, kms, ms)
        e.set_stage_timing(False)
        assert e.last_stage_ms() == [] and e.last_kernel_ms() == []
        again = e.pipeline(dev(img)).cpu().numpy()
        assert e.last_stage_ms() == []
        for got in (plain, timed, again):
            assert np.array_equal(got[0], want[stages]), stages
    # switched on once and left on across the reconfiguration: the next call reports the new stage count
    setup(4)
    e.set_stage_timing(True)
    assert np.array_equal(e.pipeline(dev(img)).cpu().numpy()[0], want[4])
    assert len(e.last_stage_ms()) == 4
    setup(2)
    assert np.array_equal(e.pipeline(dev(img)).cpu().numpy()[0], want[2])
    ms = e.last_stage_ms()
    assert len(ms) == 2 and all(v > 0 for v in ms) and len(e.last_kernel_ms()) == 2
    e.close()


# -------------------------------------------------------------------------------------------------------------- offset buffers
ROUTES = [
    ("hybrid", (2, "sdy", 4, 4), {}),
    ("tube", (2, "sdy", 4, 4), {"final_stage_kernel": 5}),
    ("gather", (2, "sdy", 4, 4), {"final_stage_kernel": 1}),
    ("x2", (2, "sdy", 2, 4), {}),
    ("scale1", (2, "sdy", 1, 4), {}),
    ("wide", (2, "sdyeho", 4, 4), {}),
    ("iv5", (2, "sdy", 4, 5), {}),
    ("iv6", (2, "sdy", 4, 6), {}),
]
SLACK, FILL = 128, 0xA5


class Offset(object):
    """n bytes at byte offset k (1..3) of a larger allocation of its own: SLACK + k owned bytes before, SLACK after, all FILL"""

    def __init__(self, n, k):
        self.big = torch.full((SLACK + k + n + SLACK,), FILL, dtype=torch.uint8, device="cuda")
        self.view = self.big[SLACK + k:SLACK + k + n]
        assert self.big.data_ptr() % 4 == 0 and self.view.data_ptr() % 4 == k
        self.lo, self.hi = SLACK + k, SLACK + k + n

    def slack_untouched(self):
        b = self.big.cpu().numpy()
        return bool((b[:self.lo] == FILL).all() and (b[self.hi:] == FILL).all())


def _call(e, what, stage, src, dst, layout, N, H, W, C):
    st = e._stream()
    if what == "pipeline":
        rc = e._lib.mulut_pipeline(e._h, src.data_ptr(), dst.data_ptr(), N, H, W, C, layout, st)
    else:
        rc = e._lib.mulut_stage(e._h, stage, src.data_ptr(), layout, dst.data_ptr(), layout, N, H, W, C, st)
    assert rc == 0, (what, stage, rc)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,cfg,tuning", ROUTES, ids=[r[0] for r in ROUTES])
def test_buffers_at_odd_addresses_give_the_same_bytes_and_nothing_outside(name, cfg, tuning):
    """mulut.h: caller buffers need no alignment.  W % 4 == 0, so a 4-aligned base takes the kernels' dword loads and stores and
    an odd base their byte paths: both must give the same bytes, and an output view at offset 1, 2, 3 must leave the bytes around
    it alone (the x4 planar store writes whole dwords)."""
    stages, modes, scale, interval = cfg
    rng = np.random.default_rng(len(name))
    e = MuLUTEngine(0).configure(*cfg)
    for s in range(1, stages + 1):
        for m in dict.fromkeys(modes):
            e.set_lut(s, m, A.make_table(rng, interval, scale * scale if s == stages else 1, True))
    for k, v in tuning.items():
        e.set_tuning(k, v)
    N, H, W = 2, 40, 72
    assert W % 4 == 0
    bad = []
    for C in (3, 1):
        img = A.natural_noise(N, H, W, C, seed=C)
        for layout in (LAYOUT_HWC, LAYOUT_CHW):
            host = to_layout(img, layout)
            for what, stage in (("pipeline", 0), ("stage", 1), ("stage", stages)):
                u = scale if what == "pipeline" or stage == stages else 1
                n_in, n_out = host.size, host.size * u * u
                ref_in, ref_out = dev(host.reshape(-1)), torch.zeros(n_out, dtype=torch.uint8, device="cuda")
                assert ref_in.data_ptr() % 4 == 0 and ref_out.data_ptr() % 4 == 0
                _call(e, what, stage, ref_in, ref_out, layout, N, H, W, C)
                want = ref_out.cpu().numpy()
                for k_in, k_out in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 2), (3, 1)):
                    src, dst = Offset(n_in, k_in), Offset(n_out, k_out)
                    src.view.copy_(ref_in)
                    _call(e, what, stage, src.view, dst.view, layout, N, H, W, C)
                    got = dst.view.cpu().numpy()
                    if not np.array_equal(got, want):
                        bad.append((what, stage, "CHW" if layout == LAYOUT_CHW else "HWC", C, k_in, k_out, "%d bytes differ" % int((got != want).sum())))
                    if not dst.slack_untouched():
                        bad.append((what, stage, "CHW" if layout == LAYOUT_CHW else "HWC", C, k_in, k_out, "bytes around the output were written"))
                    if not src.slack_untouched():
                        bad.append((what, stage, "CHW" if layout == LAYOUT_CHW else "HWC", C, k_in, k_out, "bytes around the input were written"))
    e.close()
    assert not bad, "%s: %d failures, first: %r" % (name, len(bad), bad[:10])
