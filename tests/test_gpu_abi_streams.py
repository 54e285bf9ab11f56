"""Stream order and host threads of the C ABI (-m gpu).  include/mulut.h: "all work is stream-ordered and asynchronous with respect
to the host", set-up calls wait for work in flight, "contexts may be created and first used from several host threads".

torch's side streams are non-blocking: the legacy null stream does not wait for them, nor they for it.  So an entry point that
launched on another stream than the one it was given would read input that a torch kernel queued on that stream has not written
yet -- every input below is produced that way (Late), behind a delay, while the default stream runs unrelated pipeline calls."""
import copy
import ctypes
import threading

import numpy as np
import pytest

import abi_sequences as A
import ft_exact_cases as fx

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine, metrics  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402
from oracle import c_oracle  # noqa: E402
from test_gpu_ft_exact import _ptrs, _stage_on_gpu, quantiser_weights, same_bits  # noqa: E402


class Late(object):
    """A device tensor that holds zeros until make() -- a torch kernel on the CURRENT stream, queued behind a few milliseconds of
    other work on that stream -- writes `host` into it (uint8: two's complement of the stored inverse; floats: negation, exact)."""
    _spin = None

    def __init__(self, host):
        h = torch.from_numpy(np.ascontiguousarray(host))
        self.bytes = h.dtype == torch.uint8
        self.src = (~h if self.bytes else -h).cuda()
        self.dst = torch.zeros_like(self.src)

    def make(self):
        if Late._spin is None:
            Late._spin = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
        for _ in range(16):
            Late._spin.add_(1)
        return torch.bitwise_not(self.src, out=self.dst) if self.bytes else torch.neg(self.src, out=self.dst)


@pytest.fixture(scope="module")
def busy(shipped_luts):
    """unrelated work of the library on the default stream: 1080p pipeline calls of another context, queued and not waited for"""
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(shipped_luts)
    x = torch.from_numpy(natural_frames(1, 1080, 1920, 3, seed=3)).cuda()
    out = torch.empty((1, 4320, 7680, 3), dtype=torch.uint8, device="cuda")

    def go():
        for _ in range(3):
            e.pipeline(x, out=out)
    yield go
    torch.cuda.synchronize()
    e.close()


@pytest.fixture
def side():
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    yield s
    torch.cuda.synchronize()


def test_inference_entry_points_on_a_side_stream(busy, side, shipped_luts):
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(shipped_luts)
    img = A.natural_noise(2, 45, 76, 3, seed=1)
    chw = np.ascontiguousarray(img[0].transpose(2, 0, 1))
    l2 = [shipped_luts["s2_" + m] for m in "sdy"]
    full = np.stack([c_oracle.pipeline(shipped_luts, 2, "sdy", 4, im) for im in img])
    late = {k: Late(v) for k, v in (("pass", chw), ("stage", img), ("band", img[:, 6:35]), ("chw", img.transpose(0, 3, 1, 2)))}
    torch.cuda.synchronize()
    busy()
    with torch.cuda.stream(side):
        got_pass = e.pass_q(2, "d", 3, late["pass"].make()).cpu().numpy()
        got_stage = e.stage(2, late["stage"].make()).cpu().numpy()
        got_rows = e.pipeline_rows(late["band"].make(), 6, 12, 29, 45).cpu().numpy()
        got_chw = e.pipeline(late["chw"].make(), layout=LAYOUT_CHW).cpu().numpy()
    assert np.array_equal(got_pass, c_oracle.pass_q(shipped_luts["s2_d"], chw, 3, 4, "d"))
    assert np.array_equal(got_stage, np.stack([c_oracle.stage(l2, "sdy", True, im, 4) for im in img]))
    assert np.array_equal(got_rows, full[:, 12 * 4:29 * 4])
    assert np.array_equal(got_chw, full.transpose(0, 3, 1, 2))
    e.close()


def test_detail_counters_on_a_side_stream(busy, side, shipped_luts):
    """mulut_last_detail_counters copies on the stream it is given and waits for it: asked on the side stream right after the
    pipeline call queued there, it must report that call -- the same numbers as after a device-wide wait."""
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(shipped_luts)
    img = A.natural_noise(1, 256, 320, 3, seed=4)
    late = Late(img)
    torch.cuda.synchronize()
    busy()
    with torch.cuda.stream(side):
        out = e.pipeline(late.make())
        first = e.last_detail_counters()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], c_oracle.pipeline(shipped_luts, 2, "sdy", 4, img[0]))
    e.pipeline(torch.from_numpy(img).cuda())
    torch.cuda.synchronize()
    second = e.last_detail_counters()
    assert first["items"] > 0 and sum(first["samples_per_anchor"]) > 0, first
    assert first["samples_per_anchor"] == second["samples_per_anchor"] and first["fix_pixels"] == second["fix_pixels"], (first, second)
    e.close()


def test_eval_y_on_a_side_stream(busy, side):
    rng = np.random.default_rng(8)
    gt = natural_frames(1, 300, 400, 3, seed=8)[0]
    out = np.clip(np.round(gt + rng.normal(0, 7, gt.shape)), 0, 255).astype(np.uint8)
    e = MuLUTEngine(0)
    lg, lo = Late(gt), Late(out)
    torch.cuda.synchronize()
    busy()
    with torch.cuda.stream(side):
        p, s = e.eval_y(lg.make(), lo.make(), 4)
    y_gt, y_out = metrics.rgb2ycbcr(gt)[:, :, 0], metrics.rgb2ycbcr(out)[:, :, 0]
    assert p == pytest.approx(float(metrics.psnr(y_gt, y_out, 4)), abs=1e-4)      # the bars of test_gpu_eval.py
    assert s == pytest.approx(metrics.ssim(y_gt, y_out), abs=1e-10)
    e.close()


def test_quantiser_on_a_side_stream(busy, side):
    from mulut_amd import _native
    lib = _native.load()
    M, n = 3, 6561 * 16
    w = quantiser_weights(M, n, 77)
    g = np.random.default_rng(5).standard_normal((M, n)).astype(np.float32)
    r = torch.round(torch.from_numpy(w) * 127)
    want_fwd = torch.clamp(r, -127, 127).numpy()
    want_bwd = (torch.from_numpy(g) * ((r >= -127) & (r <= 127)) * 127).numpy()
    lw, lg = [Late(w[m]) for m in range(M)], [Late(g[m]) for m in range(M)]
    torch.cuda.synchronize()
    busy()
    with torch.cuda.stream(side):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert st.value == side.cuda_stream
        ws, grads = [x.make() for x in lw], [x.make() for x in lg]
        outs = [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(M)]
        assert lib.mulut_ft_quantize(0, _ptrs(ws), _ptrs(outs), M, n, st) == 0
        assert lib.mulut_ft_quantize_backward(0, _ptrs(ws), _ptrs(grads), M, n, st) == 0
        got_f, got_b = [o.cpu().numpy() for o in outs], [x.cpu().numpy() for x in grads]
    for m in range(M):
        assert same_bits(got_f[m], want_fwd[m]) and same_bits(got_b[m], want_bwd[m]), m


FT_CASES = [c for c in fx.CASES if c.modes == "sdy" and c.content == "noise" and c.tables_kind == "rand" and
            c.shape in ((2, 1, 13, 10), (1, 2, 9, 11)) and c.u in (1, 4)]
# checked when the file is imported, so also by a collection without a GPU: intervals 4, 5 and 6, final x4 and non-final stages
assert {(c.interval, c.u, c.last) for c in FT_CASES} >= {(iv, u, last) for iv in (4, 5, 6) for u, last in ((4, 1), (1, 0))}


def _reference_and_inputs(case, late):
    """(reference, tables, x, gout as `late` makes them) of a case.  The case objects are those of ft_exact_cases.CASES, which
    ft_abi_cases.built() caches, built, for the whole process: the arrays are built on a copy, and only the copy's are released."""
    own = copy.copy(case).build()
    try:
        return fx.reference(own), [late(t.astype(np.float32)) for t in own.tables], late(own.x), late(own.gout)
    finally:
        own.tables = own.x = own.gout = None


@pytest.mark.parametrize("case", FT_CASES, ids=lambda c: c.name)
def test_fine_tune_stage_entry_points_on_a_side_stream(busy, side, case):
    """mulut_ft_stage_forward(_mask) / backward(_mask) at interval 4, mulut_ft_interval_stage_forward / backward at 5 and 6, on the
    integer cases of tests/ft_exact_cases.py: exact, so np.array_equal applies."""
    from mulut_amd import _native
    lib = _native.load()
    ref, lw, lx, lg = _reference_and_inputs(case, Late)
    torch.cuda.synchronize()
    busy()
    bad = []
    with torch.cuda.stream(side):
        wq, x, gout = [t.make() for t in lw], lx.make(), lg.make()
        inside = None
        forms = (False, True) if case.interval == 4 else (True,)
        for masked in forms:
            out, mask = _stage_on_gpu(lib, case, wq, x, gout, masked)
            bad.append(fx.describe(case, "out (masked %s)" % masked, out, ref.out, q=1))
            if masked:
                bits = mask & np.uint16((1 << case.u * case.u) - 1)
                bad.append(fx.describe(case, "inside", bits.astype(np.float32), ref.inside.astype(np.int64), q=1))
                inside = torch.from_numpy(mask.view(np.int16)).cuda()
        for masked in forms:
            gx, gw = _stage_on_gpu(lib, case, wq, x, gout, masked, inside)
            bad.append(fx.describe(case, "grad_x (masked %s)" % masked, gx, ref.gx_num))
            for m in range(case.M):
                bad.append(fx.describe(case, "grad_wq[%d] (masked %s)" % (m, masked), gw[m], ref.gw_num[m]))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------- a table rewrite against queued work
def _windows(out_frame, ref_fn, frame, H, W):
    for (y, x) in ((0, 0), (500, 900), (H - 96, W - 96)):
        y0, y1, x0, x1 = max(0, y - 4), min(H, y + 100), max(0, x - 4), min(W, x + 100)
        ref = ref_fn(frame[y0:y1, x0:x1])[(y - y0) * 4:(y - y0 + 96) * 4, (x - x0) * 4:(x - x0 + 96) * 4]
        assert np.array_equal(out_frame[y * 4:(y + 96) * 4, x * 4:(x + 96) * 4].cpu().numpy(), ref), (y, x)


def test_set_lut_waits_for_pipeline_calls_still_queued(shipped_luts):
    """mulut_set_lut rewrites a table of the same shape in place, from the host, outside any stream of the caller.  Pipeline calls
    queued on a non-blocking stream and not yet run must still see the OLD rows: mulut_set_lut waits for the device before it
    touches a table (wait_for_device in mulut_capi.hip; the header states it).  Six calls of eight 1080p frames (0.8 GB of output
    each, one buffer) are in flight -- the event recorded behind them has not fired -- when the final stage's three tables are
    replaced.
    Without the wait the copy is ordered against nothing the caller has queued: a synchronous hipMemcpy runs on the
    null stream, which non-blocking streams do not wait for.  Observed on the MI355X: with the library of the commit before the
    wait, and with the wait taken out of mulut_set_lut alone, this test fails with 794,697,968 of 796,262,400 bytes differing --
    nearly all six queued calls ran on the new rows.  The paths that FREE memory (a table of another size, an interval
    change, a growing work list, mulut_destroy) take the same wait and are settled by reading the code: they are never raced on the device."""
    H, W = 1080, 1920
    nat = natural_frames(2, H, W, 3, seed=6)
    noise = np.random.default_rng(6).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    frames = np.stack([nat[0], noise[0], nat[1], noise[1]] * 2)
    new_luts = dict(shipped_luts)
    for m in "sdy":
        new_luts["s2_" + m] = np.clip(-shipped_luts["s2_" + m].astype(np.int16), -128, 127).astype(np.int8)
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(shipped_luts)
    batch = torch.from_numpy(frames).cuda()
    old = e.pipeline(batch)
    torch.cuda.synchronize()
    for n in (0, 1):        # tie the engine's own result to the oracle (as test_full_1080p_frame does)
        _windows(old[n], lambda im: c_oracle.pipeline(shipped_luts, 2, "sdy", 4, im), frames[n], H, W)
    out = torch.zeros_like(old)
    side = torch.cuda.Stream()
    done = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(6):
            e.pipeline(batch, out=out)
        done.record(side)
    in_flight = not done.query()
    for m in "sdy":
        e.set_lut(2, m, new_luts["s2_" + m])
    torch.cuda.synchronize()
    assert in_flight, "the queued calls had finished before the tables were replaced: nothing was tested"
    assert torch.equal(out, old), "queued pipeline calls read rows of the NEW tables: %d bytes differ" % int((out != old).sum())
    new = e.pipeline(batch)
    torch.cuda.synchronize()
    assert not torch.equal(new[0], old[0])
    for n in (0, 1):
        _windows(new[n], lambda im: c_oracle.pipeline(new_luts, 2, "sdy", 4, im), frames[n], H, W)
    e.close()


# ------------------------------------------------------------------------------------------------------------------ host threads
THREAD_CONFIGS = [(2, "sdy", 4, 4), (2, "sdy", 3, 4), (1, "eho", 4, 4), (2, "sdy", 4, 6)]


def test_contexts_created_and_first_used_from_four_host_threads():
    """mulut.h: the one-time per-device set-ups (raising each kernel's dynamic-LDS limit on its first launch) are serialised inside
    the library, so contexts may be created and first used from several host threads.  Four threads, each with its own stream and
    its own route family, create their contexts at the same moment and run their first and second pipeline call.  One round:
    this checks the documented contract, it does not try to provoke a failure."""
    rng = np.random.default_rng(12)
    jobs = []
    assert len({A.family_of(*cfg) for cfg in THREAD_CONFIGS}) == len(THREAD_CONFIGS) == 4      # four different route families
    for k, (stages, modes, scale, interval) in enumerate(THREAD_CONFIGS):
        tables = {(s, m): A.make_table(rng, interval, scale * scale if s == stages else 1, True)
                  for s in range(1, stages + 1) for m in dict.fromkeys(modes)}
        imgs = [A.natural_noise(1, 40, 68, 3, seed=20 + 2 * k + j) for j in range(2)]
        want = [A.ref_pipeline(tables, stages, modes, scale, im[0], interval) for im in imgs]
        jobs.append((stages, modes, scale, interval, tables, imgs, want))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in jobs]
    barrier = threading.Barrier(len(jobs))
    errors, results = [None] * len(jobs), [None] * len(jobs)

    def work(k):
        try:
            stages, modes, scale, interval, tables, imgs, _ = jobs[k]
            with torch.cuda.stream(streams[k]):
                xs = [torch.from_numpy(im).cuda() for im in imgs]
                barrier.wait(timeout=60)
                e = MuLUTEngine(0)
                e.configure(stages, modes, scale, interval)
                for (s, m), t in tables.items():
                    e.set_lut(s, m, t)
                results[k] = [e.pipeline(x).cpu().numpy() for x in xs]
                e.close()
        except BaseException as ex:      # noqa: B036  (re-raised in the main thread)
            errors[k] = ex
            barrier.abort()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads)
    for ex in errors:
        if ex is not None:
            raise ex
    for k, job in enumerate(jobs):
        for j in range(2):
            assert np.array_equal(results[k][j][0], job[6][j]), (THREAD_CONFIGS[k], "call %d" % j)
