"""The fine-tune half of include/mulut.h held to its buffer and stream contracts (-m gpu): mulut_ft_quantize(_backward), the four
families of mulut_ft*_stage_forward / _backward, mulut_eval_y.

Every case is an exact-integer case (tests/ft_abi_cases.py: integer tables, integer x, grad_out = avg * k), so every output is the
oracle's bytes in any summation order and the tests assert equality, no float bar (premises: tests/test_ft_abi_cpu.py).
  1. arena       every pointer of a call carved out of one allocation at 4, 8 and 12 bytes past a 16-byte boundary (`inside` 2 bytes
                 past a 4-byte one), poisoned slack on both sides of every buffer: the reference's values, the bytes of the
                 16-aligned run, and not one byte changed outside the outputs;
  2. accumulate  grad_wq and grad_x prefilled in every element: prefill + reference, and prefill + 2 * reference after a second call;
  3. streams     producer, forward, backward, quantiser backward and consumer queued on a non-blocking stream without a wait between;
  4. capture     the same chain captured into a graph after a warm-up, replayed, inputs rewritten in place, replayed again;
  5. the module's refusals and equivalences, and the interval-4 kernels on pixels outside 0..255, infinite and NaN."""
import copy
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ft_abi_cases as fa            # noqa: E402
import ft_exact_cases as fx          # noqa: E402
import ft_wide_cases as fw           # noqa: E402
from test_gpu_ft_exact import quantiser_weights, same_bits      # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from mulut_amd import _native
    return _native.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


class DevArena(object):
    """a fa.Arena on the device: one uint8 allocation (torch aligns it to 512 bytes), every buffer a pointer into it"""

    def __init__(self, plan, contents):
        self.plan = plan
        self.before = plan.image(contents)
        self.buf = torch.from_numpy(self.before).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self, name):
        return self.buf.data_ptr() + self.plan.offset(name)

    def ptrs(self, prefix, M):
        return _ptr_array([self.ptr("%s%d" % (prefix, m)) for m in range(M)])

    def read(self):
        return self.buf.cpu().numpy()


class Ptrs(object):
    """the pointers of a stage call, from an arena or from torch tensors"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def forward(lib, case, entry, p, stream=None):
    B, C, H, W = case.shape
    st = stream or _stream()
    head = (p.wq, case.modes.encode(), case.last, case.u, p.x, B, C, H, W, p.out)
    if entry == "plain":
        rc = lib.mulut_ft_stage_forward(0, *head, st)
    elif entry == "mask":
        rc = lib.mulut_ft_stage_forward_mask(0, *head, p.inside, st)
    elif entry == "interval":
        rc = lib.mulut_ft_interval_stage_forward(0, case.interval, *head, p.inside, st)
    else:
        rc = lib.mulut_ft_wide_stage_forward(0, case.interval, *head, p.inside, st)
    assert rc == 0, (entry, rc)


def backward(lib, case, entry, p, stream=None):
    B, C, H, W = case.shape
    st = stream or _stream()
    head = (p.wq, case.modes.encode(), case.last, case.u, p.x, p.gout)
    tail = (B, C, H, W, p.gw, p.gx, st)
    if entry == "plain":
        rc = lib.mulut_ft_stage_backward(0, *head, *tail)
    elif entry == "mask":
        rc = lib.mulut_ft_stage_backward_mask(0, *head, p.inside, *tail)
    elif entry == "interval":
        rc = lib.mulut_ft_interval_stage_backward(0, case.interval, *head, p.inside, *tail)
    else:
        rc = lib.mulut_ft_wide_stage_backward(0, case.interval, *head, p.inside, *tail)
    assert rc == 0, (entry, rc)


def arena_ptrs(ar, case, backward_call, with_mask):
    p = Ptrs(x=ar.ptr("x"), wq=ar.ptrs("wq", case.M), inside=ar.ptr("inside") if with_mask else None)
    if backward_call:
        p.gout, p.gw, p.gx = ar.ptr("gout"), ar.ptrs("gw", case.M), ar.ptr("gx")
    else:
        p.out = ar.ptr("out")
    return p


def inputs_of(case, x=None, gout=None):
    c = {"x": case.x if x is None else x, "gout": case.gout if gout is None else gout}
    for m in range(case.M):
        c["wq%d" % m] = case.tables[m].astype(np.float32)
    return c


def run_forward(lib, case, ref, entry, k, x=None):
    """one forward in an arena at offset k: (out, inside bits or None, what changed outside the outputs)"""
    B, C, H, W = case.shape
    with_mask = entry != "plain"
    plan = fa.stage_arena(case, k, False, with_mask)
    c = {n: v for n, v in inputs_of(case, x=x).items() if n != "gout"}
    c["out"] = np.full(B * C * H * W * case.u * case.u, np.nan, np.float32)
    if with_mask:
        c["inside"] = np.full(B * C * H * W, 0xFFFF, np.uint16)
    ar = DevArena(plan, c)
    forward(lib, case, entry, arena_ptrs(ar, case, False, with_mask))
    after = ar.read()
    bad = plan.outside_changed(ar.before, after, ("out", "inside"))
    out = plan.get(after, "out", np.float32).reshape(B, C, H * case.u, W * case.u)
    bits = plan.get(after, "inside", np.uint16).reshape(case.shape) & np.uint16((1 << case.u * case.u) - 1) if with_mask else None
    return out, bits, bad


def run_backward(lib, case, ref, entry, k, pre=None, calls=1, x=None, gout=None):
    """`calls` backward calls in one arena at offset k, the gradients zero or prefilled: (grad_x, [grad_wq], what changed outside)"""
    with_mask = entry != "plain"
    plan = fa.stage_arena(case, k, True, with_mask)
    c = inputs_of(case, x=x, gout=gout)
    if with_mask:
        c["inside"] = ref.inside.astype(np.uint16)
    rows, el = fa.rows_of(case.interval), case.u * case.u
    for m in range(case.M):
        c["gw%d" % m] = fa.as_f32(pre[0][m], case.q) if pre else np.zeros((rows, el), np.float32)
    c["gx"] = fa.as_f32(pre[1], case.q) if pre else np.zeros(case.shape, np.float32)
    ar = DevArena(plan, c)
    p = arena_ptrs(ar, case, True, with_mask)
    for _ in range(calls):
        backward(lib, case, entry, p)
    after = ar.read()
    bad = plan.outside_changed(ar.before, after, ["gx"] + ["gw%d" % m for m in range(case.M)])
    gx = plan.get(after, "gx", np.float32).reshape(case.shape)
    gw = [plan.get(after, "gw%d" % m, np.float32).reshape(rows, el) for m in range(case.M)]
    return gx, gw, bad


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


CASE_ENTRIES = [(c, e) for c in fa.CASES for e in fa.entries_of(c)]
_ids = ["%s-%s" % (c.name, e) for c, e in CASE_ENTRIES]


# ------------------------------------------------------------------------------------------------------------------- 1. arena
@pytest.mark.parametrize("case,entry", CASE_ENTRIES, ids=_ids)
def test_buffers_in_an_arena_give_the_reference_bytes_and_nothing_outside(case, entry):
    lib = _lib()
    case, ref = fa.built(case)
    bad, first = [], {}
    for k in fa.OFFSETS:
        out, bits, outside = run_forward(lib, case, ref, entry, k)
        bad += ["forward, offset %d: %s" % (k, b) for b in outside]
        bad.append(fx.describe(case, "out (offset %d)" % k, out, ref.out, q=1))
        if bits is not None:
            bad.append(fx.describe(case, "inside (offset %d)" % k, bits.astype(np.float32), ref.inside.astype(np.int64), q=1))
        gx, gw, outside = run_backward(lib, case, ref, entry, k)
        bad += ["backward, offset %d: %s" % (k, b) for b in outside]
        bad.append(fx.describe(case, "grad_x (offset %d)" % k, gx, ref.gx_num))
        for m in range(case.M):
            bad.append(fx.describe(case, "grad_wq[%d] (offset %d)" % (m, k), gw[m], ref.gw_num[m]))
        got = [out, gx] + gw + ([bits] if bits is not None else [])
        if k == 0:
            first = got
        else:
            bad += ["offset %d: result %d differs in its bytes from the 16-aligned run" % (k, i) for i, (a, b) in enumerate(zip(got, first))
                    if not same_bytes(a, b)]
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("n", fa.QUANT_N)
@pytest.mark.parametrize("M", fa.QUANT_M)
def test_quantiser_pair_in_an_arena(M, n):
    lib = _lib()
    w = quantiser_weights(M, n, 2000 * M + n % 991)
    g = np.random.default_rng(n + 7 * M).standard_normal((M, n)).astype(np.float32)
    r = torch.round(torch.from_numpy(w) * 127)
    want_fwd = torch.clamp(r, -127, 127).numpy()
    want_bwd = (torch.from_numpy(g) * ((r >= -127) & (r <= 127)) * 127).numpy()
    first = None
    for k in fa.OFFSETS:
        plan = fa.Arena()
        for m in range(M):
            plan.add("w%d" % m, 4 * n, "in", 16, k)
        for m in range(M):
            plan.add("o%d" % m, 4 * n, "out", 16, k)
        for m in range(M):
            plan.add("g%d" % m, 4 * n, "out", 16, k)
        c = {}
        for m in range(M):
            c["w%d" % m], c["o%d" % m], c["g%d" % m] = w[m], np.full(n, 7.0, np.float32), g[m]
        ar = DevArena(plan, c)
        assert lib.mulut_ft_quantize(0, ar.ptrs("w", M), ar.ptrs("o", M), M, n, _stream()) == 0
        assert lib.mulut_ft_quantize_backward(0, ar.ptrs("w", M), ar.ptrs("g", M), M, n, _stream()) == 0
        after = ar.read()
        assert plan.outside_changed(ar.before, after, ["o%d" % m for m in range(M)] + ["g%d" % m for m in range(M)]) == [], k
        got_f = np.stack([plan.get(after, "o%d" % m, np.float32) for m in range(M)])
        got_b = np.stack([plan.get(after, "g%d" % m, np.float32) for m in range(M)])
        assert same_bits(got_f, want_fwd) and same_bits(got_b, want_bwd), k
        if k == 0:
            first = (got_f, got_b)
        else:
            assert same_bytes(got_f, first[0]) and same_bytes(got_b, first[1]), k


@pytest.mark.parametrize("shave", fa.EVAL_SHAVES)
@pytest.mark.parametrize("H,W", fa.EVAL_SHAPES)
def test_eval_y_in_an_arena(H, W, shave):
    """one window (11 x 11), a second tile of one column (11 x 43) and of one row (43 x 11): the images at odd addresses, the
    workspace 8 bytes past a 16-byte boundary and 16-aligned; the bars of test_gpu_eval.py"""
    from mulut_amd import metrics
    from mulut_amd.synth import natural_frames
    lib = _lib()
    rng = np.random.default_rng(100 * H + W)
    gt = np.ascontiguousarray(natural_frames(1, 64, 64, 3, seed=H + W)[0][:H, :W])
    out = np.clip(np.round(gt + rng.normal(0, 7, gt.shape)), 0, 255).astype(np.uint8)
    y_gt, y_out = metrics.rgb2ycbcr(gt)[:, :, 0], metrics.rgb2ycbcr(out)[:, :, 0]
    want_p, want_s = float(metrics.psnr(y_gt, y_out, shave)), metrics.ssim(y_gt, y_out)
    n = int(lib.mulut_eval_ws_doubles(H, W))
    for k_img, k_ws in ((1, 8), (3, 0), (0, 8)):
        plan = fa.Arena().add("gt", gt.size, "in", 16, k_img).add("out", out.size, "in", 16, (k_img + 6) % 16).add("ws", 8 * n, "out", 16, k_ws)
        ar = DevArena(plan, {"gt": gt, "out": out, "ws": np.full(n, np.nan, np.float64)})
        p, s = ctypes.c_double(), ctypes.c_double()
        rc = lib.mulut_eval_y(0, ar.ptr("gt"), ar.ptr("out"), H, W, shave, ar.ptr("ws"), n, ctypes.byref(p), ctypes.byref(s), _stream())
        assert rc == 0, rc
        assert plan.outside_changed(ar.before, ar.read(), ("ws",)) == [], (k_img, k_ws)
        assert p.value == pytest.approx(want_p, abs=1e-4), (k_img, k_ws)
        assert s.value == pytest.approx(want_s, abs=1e-10), (k_img, k_ws)


# -------------------------------------------------------------------------------------------------------------- 2. accumulate
@pytest.mark.parametrize("case,entry", CASE_ENTRIES, ids=_ids)
def test_backward_adds_into_prefilled_gradients_once_and_twice(case, entry):
    """'accumulates ... into grad_wq': every element of grad_wq and grad_x prefilled with seeded integers over q.  One call gives
    prefill + reference, a second call without zeroing prefill + 2 * reference; elements the case does not touch come back as they
    were.  A store where an add belongs, or a flush that skips a sum equal to what is there, shows in the first call already."""
    lib = _lib()
    case, ref = fa.built(case)
    assert fa.accumulate_cap(case, ref, calls=2) < fa.CAP
    pre = fa.prefill(case)
    bad = []
    for calls in (1, 2):
        gx, gw, outside = run_backward(lib, case, ref, entry, 4, pre=pre, calls=calls)
        bad += ["%d call(s): %s" % (calls, b) for b in outside]
        bad.append(fx.describe(case, "grad_x after %d call(s) into a prefilled buffer" % calls, gx, pre[1] + calls * ref.gx_num))
        for m in range(case.M):
            bad.append(fx.describe(case, "grad_wq[%d] after %d call(s) into a prefilled buffer" % (m, calls), gw[m], pre[0][m] + calls * ref.gw_num[m]))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------------------------ 3. streams
SPIN_BYTES, SPIN_OPS = 256 << 20, 16      # the producer's delay, sized as Late of test_gpu_abi_streams.py: 16 passes over 256 MiB
_spin = {}


def spin():
    if "buf" not in _spin:
        _spin["buf"] = torch.zeros(SPIN_BYTES, dtype=torch.uint8, device="cuda")
    for _ in range(SPIN_OPS):
        _spin["buf"].add_(1)


def float_weights(case):
    """float parameters whose quantisation is the case's integer tables: t / 127, and beyond the quantiser's clamp (+-128 / 127, which
    rounds to +-128 and is clamped to +-127) at half of the entries that are +-127 -- there the quantiser's backward stops the gradient.
    Returns (weights, inside): inside = round(w * 127) within [-127, 127], computed by torch on the host."""
    rng = np.random.default_rng(len(case.name))
    ws, ins = [], []
    for t in case.tables:
        w = (t / 127.0).astype(np.float32)
        beyond = (np.abs(t) == 127) & (rng.random(t.shape) < 0.5)
        w[beyond] = (np.sign(t[beyond]) * 128 / 127.0).astype(np.float32)
        r = torch.round(torch.from_numpy(w) * 127)
        assert np.array_equal(torch.clamp(r, -127, 127).numpy(), t.astype(np.float32)) and beyond.any()
        inside = ((r >= -127) & (r <= 127)).numpy()
        assert np.array_equal(~inside, beyond)
        ws.append(w)
        ins.append(inside)
    return ws, ins


class Chain(object):
    """static device buffers of the chain forward_mask -> backward -> quantize_backward for one shape, and the chain itself"""

    def __init__(self, case, entry):
        B, C, H, W = case.shape
        u, rows, el = case.u, fa.rows_of(case.interval), case.u * case.u
        f32 = dict(dtype=torch.float32, device="cuda")
        self.case, self.entry = case, entry
        self.x = torch.zeros(case.shape, **f32)
        self.wq = [torch.zeros((rows, el), **f32) for _ in range(case.M)]
        self.w = [torch.zeros((rows, el), **f32) for _ in range(case.M)]
        self.gout = torch.zeros((B, C, H * u, W * u), **f32)
        self.out = torch.full((B, C, H * u, W * u), float("nan"), **f32)
        self.inside = torch.full(case.shape, -1, dtype=torch.int16, device="cuda")
        self.gw = [torch.zeros((rows, el), **f32) for _ in range(case.M)]
        self.gx = torch.zeros(case.shape, **f32)

    def load(self, case, weights, late=False):
        """the content of `case` into the static buffers, in place; late: x and the tables are left to produce()"""
        self.gout.copy_(torch.from_numpy(case.gout))
        for m in range(case.M):
            self.w[m].copy_(torch.from_numpy(weights[m]))
        self.src_x = torch.from_numpy(-case.x).cuda()
        self.src_wq = [torch.from_numpy(-t.astype(np.float32)).cuda() for t in case.tables]
        if not late:
            self.produce()

    def produce(self):
        torch.neg(self.src_x, out=self.x)
        for s, d in zip(self.src_wq, self.wq):
            torch.neg(s, out=d)

    def ptrs(self):
        return Ptrs(x=self.x.data_ptr(), wq=_ptr_array([t.data_ptr() for t in self.wq]), gout=self.gout.data_ptr(), out=self.out.data_ptr(),
                    inside=self.inside.data_ptr(), gw=_ptr_array([t.data_ptr() for t in self.gw]), gx=self.gx.data_ptr())

    def zero(self):
        for t in self.gw:
            t.zero_()
        self.gx.zero_()

    def calls(self, lib):
        """forward_mask, backward, quantize_backward on the current stream, nothing waited for"""
        p, st, case = self.ptrs(), _stream(), self.case
        forward(lib, case, self.entry, p, st)
        backward(lib, case, self.entry, p, st)
        rows, el = fa.rows_of(case.interval), case.u * case.u
        rc = lib.mulut_ft_quantize_backward(0, _ptr_array([t.data_ptr() for t in self.w]), p.gw, case.M, rows * el, st)
        assert rc == 0, rc

    def results(self):
        return [self.out.clone(), self.inside.clone(), self.gx.clone()] + [t.clone() for t in self.gw]

    def check(self, res, case, ref, q_inside, what):
        res = [t.cpu().numpy() for t in res]
        bits = res[1].view(np.uint16) & np.uint16((1 << case.u * case.u) - 1)
        bad = [fx.describe(case, "%s: out" % what, res[0], ref.out, q=1),
               fx.describe(case, "%s: inside" % what, bits.astype(np.float32), ref.inside.astype(np.int64), q=1),
               fx.describe(case, "%s: grad_x" % what, res[2], ref.gx_num)]
        for m in range(case.M):      # the quantiser's backward: x 127 inside its clamp, 0 beyond
            bad.append(fx.describe(case, "%s: grad of weight %d" % (what, m), res[3 + m], ref.gw_num[m] * 127 * q_inside[m]))
        return [b for b in bad if b]


@pytest.mark.parametrize("key", sorted(fa.FAMILY_CASES))
def test_calls_queued_behind_their_producer_on_a_side_stream(key):
    """x and the tables are written by torch kernels on a non-blocking stream, behind a delay; forward_mask, backward,
    quantize_backward and a consumer that copies the results are queued on that stream right behind them, nothing waited for until
    the end.  A launch on any other stream would read the zeros the buffers held before.  The default stream runs unrelated work
    on a buffer of its own meanwhile."""
    lib = _lib()
    case, ref = fa.built(fa.FAMILY_CASES[key])
    weights, q_inside = float_weights(case)
    chain = Chain(case, fa.FAMILY_ENTRY[key])
    chain.load(case, weights)
    chain.calls(lib)                       # warm-up: the first launch of a kernel raises its LDS limit
    torch.cuda.synchronize()
    chain.x.zero_()
    for t in chain.wq:
        t.zero_()
    chain.zero()
    chain.out.fill_(float("nan"))
    chain.inside.fill_(-1)
    unrelated = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    side, produced = torch.cuda.Stream(), torch.cuda.Event()
    torch.cuda.synchronize()
    for _ in range(8):
        unrelated.add_(1)                  # the default stream, busy and unrelated
    with torch.cuda.stream(side):
        assert _stream().value == side.cuda_stream
        spin()
        chain.produce()
        produced.record(side)
        chain.calls(lib)
        res = chain.results()
        in_flight = not produced.query()
        side.synchronize()
    torch.cuda.synchronize()
    assert in_flight, "the producer had finished before the calls were queued: nothing was tested"
    bad = chain.check(res, case, ref, q_inside, "side stream")
    assert not bad, "\n".join(bad)
    assert bool((unrelated == 8).all())


def test_eval_y_queued_behind_its_producer_on_a_side_stream():
    from mulut_amd import metrics
    from mulut_amd.synth import natural_frames
    lib = _lib()
    H, W, shave = 43, 11, 0
    gt = np.ascontiguousarray(natural_frames(1, 64, 64, 3, seed=5)[0][:H, :W])
    out = np.clip(np.round(gt + np.random.default_rng(5).normal(0, 7, gt.shape)), 0, 255).astype(np.uint8)
    y_gt, y_out = metrics.rgb2ycbcr(gt)[:, :, 0], metrics.rgb2ycbcr(out)[:, :, 0]
    src = [torch.from_numpy(~a).cuda() for a in (gt, out)]
    dst = [torch.zeros_like(s) for s in src]
    n = int(lib.mulut_eval_ws_doubles(H, W))
    ws = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    unrelated = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    side, produced = torch.cuda.Stream(), torch.cuda.Event()
    spin()                                 # (allocates the spin buffer on first use, outside the timed window)
    torch.cuda.synchronize()
    for _ in range(8):
        unrelated.add_(1)
    p, s = ctypes.c_double(), ctypes.c_double()
    with torch.cuda.stream(side):
        spin()
        for a, b in zip(src, dst):
            torch.bitwise_not(a, out=b)
        produced.record(side)
        in_flight = not produced.query()      # (asked before the call: mulut_eval_y waits for its stream before it returns)
        rc = lib.mulut_eval_y(0, dst[0].data_ptr(), dst[1].data_ptr(), H, W, shave, ws.data_ptr(), n, ctypes.byref(p), ctypes.byref(s), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert in_flight, "the producer had finished before mulut_eval_y was called: nothing was tested"
    assert p.value == pytest.approx(float(metrics.psnr(y_gt, y_out, shave)), abs=1e-4)
    assert s.value == pytest.approx(metrics.ssim(y_gt, y_out), abs=1e-10)
    assert bool((unrelated == 8).all())


# ------------------------------------------------------------------------------------------------------------------ 4. capture
@pytest.mark.parametrize("key", sorted(fa.FAMILY_CASES))
def test_a_warmed_up_chain_is_captured_and_replays_on_inputs_rewritten_in_place(key):
    """zero_() of the gradients, forward_mask, backward, quantize_backward: a linear graph on static buffers, captured after one
    eager run of the same calls.  The replay gives the reference of the first content; x, grad_out, the tables and the weights are
    then rewritten in place with a second content of the same shape and the replay gives the reference of that -- and both equal
    the eager calls, byte for byte."""
    lib = _lib()
    first, ref1 = fa.built(fa.FAMILY_CASES[key])
    second, ref2 = fa.built(fa.SECOND[key])
    w1, in1 = float_weights(first)
    w2, in2 = float_weights(second)
    chain = Chain(first, fa.FAMILY_ENTRY[key])
    chain.load(first, w1)
    chain.zero()
    chain.calls(lib)                       # the warm-up, and the eager result of the first content
    torch.cuda.synchronize()
    eager1 = chain.results()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain.zero()
        chain.calls(lib)
    torch.cuda.synchronize()
    chain.out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    got1 = chain.results()
    chain.load(second, w2)                 # in place: the graph holds the buffers' addresses
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got2 = chain.results()
    chain.zero()
    chain.calls(lib)
    torch.cuda.synchronize()
    eager2 = chain.results()
    bad = chain.check(got1, first, ref1, in1, "first replay") + chain.check(got2, second, ref2, in2, "replay on rewritten inputs")
    assert not bad, "\n".join(bad)
    for got, eager, what in ((got1, eager1, "first"), (got2, eager2, "second")):
        for i, (a, b) in enumerate(zip(got, eager)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "%s replay, result %d differs from the eager calls" % (what, i)
    assert not torch.equal(got1[0], got2[0])


# ------------------------------------------------------------------------------------------------------------------- 5. module
def _net(tmp_path, stages=2, modes="sd", scale=2, interval=4, seed=3):
    from mulut_amd.finetune import MuLUT
    rng = np.random.default_rng(seed)
    rows = fa.rows_of(interval)
    for s in range(stages):
        for m in modes:
            np.save(tmp_path / ("LUT_x%d_%dbit_int8_s%d_%s.npy" % (scale, interval, s + 1, m)),
                    rng.integers(-127, 128, (rows, scale * scale if s + 1 == stages else 1), dtype=np.int8))
    return MuLUT(str(tmp_path), stages, modes, upscale=scale, interval=interval).cuda()


def _x(shape, seed=1):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape).astype(np.float32) / np.float32(255)).cuda()


def test_module_refuses_wrong_types_and_devices_before_any_library_call(tmp_path):
    from mulut_amd.finetune import _StageFn
    net = _net(tmp_path)
    x = _x((1, 1, 6, 5))
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(TypeError):
            net(x.to(dtype))
    # (the module multiplies by 255.0 first, as the reference does, which makes a uint8 x float32: the stage function itself is asked)
    w = [net.weight_s1_s, net.weight_s1_d]
    for bad in (x.to(torch.uint8), x.to(torch.float16), x.to(torch.float64)):
        with pytest.raises(TypeError):
            _StageFn.apply(bad, "sd", False, 1, 4, *w)
    with pytest.raises(TypeError):
        _StageFn.apply(x.cpu(), "sd", False, 1, 4, *w)
    net.weight_s1_d.data = net.weight_s1_d.data.cpu()
    with pytest.raises(ValueError):
        net(x)


def _apply_stage(case, weights, x):
    """the module's stage function on leaf tensors: (x, weights, out)"""
    from mulut_amd.finetune import _StageFn
    ws = [torch.from_numpy(w).cuda().requires_grad_(True) for w in weights]
    x = x.detach().requires_grad_(True)
    return x, ws, _StageFn.apply(x, case.modes, bool(case.last), case.u, case.interval, *ws)


def _stage_want(case, ref, q_inside):
    """out, grad_x and the weights' gradients (x 127 inside the quantiser's clamp, 0 beyond) of the exact case, as float32"""
    return [ref.out.astype(np.float32), fa.as_f32(ref.gx_num, case.q)] + [fa.as_f32(ref.gw_num[m] * 127 * q_inside[m], case.q) for m in range(case.M)]


MODULE_KEYS = ["iv4_u4", "iv6_u2", "wide"]      # (exact cases: sums of atomics are then the same bytes on every run, so results can be compared as bytes)


@pytest.mark.parametrize("key", MODULE_KEYS)
def test_stage_function_on_non_contiguous_x_and_grad_out_gives_the_bytes_of_contiguous_copies(key):
    case, ref = fa.built(fa.FAMILY_CASES[key])
    weights, q_inside = float_weights(case)
    B, C, H, W = case.shape
    wide = torch.full((B, C + 2, H, W), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, 1:1 + C] = torch.from_numpy(case.x).cuda()
    xs = wide[:, 1:1 + C]                                # a channel slice of a wider tensor
    gout = torch.from_numpy(case.gout).cuda()
    assert not xs.is_contiguous()
    res = []
    for permuted in (True, False):
        x, ws, out = _apply_stage(case, weights, xs if permuted else xs.contiguous())
        if permuted:
            out.permute(0, 1, 3, 2).backward(gout.permute(0, 1, 3, 2).contiguous())      # autograd hands the stage a transposed view
        else:
            out.backward(gout)
        res.append([out.detach().cpu().numpy(), x.grad.cpu().numpy()] + [w.grad.cpu().numpy() for w in ws])
    for i, (a, b, want) in enumerate(zip(res[0], res[1], _stage_want(case, ref, q_inside))):
        assert same_bytes(a, b), i
        assert np.array_equal(a, want), i


@pytest.mark.parametrize("key", MODULE_KEYS)
def test_stage_function_without_grad_and_backward_twice(key):
    case, ref = fa.built(fa.FAMILY_CASES[key])
    weights, q_inside = float_weights(case)
    x, ws, out = _apply_stage(case, weights, torch.from_numpy(case.x).cuda())
    with torch.no_grad():
        _, _, out_ng = _apply_stage(case, weights, x)
    from mulut_amd.finetune import _StageFn
    out_nr = _StageFn.apply(x.detach(), case.modes, bool(case.last), case.u, case.interval, *[w.detach() for w in ws])
    assert torch.equal(out_ng, out.detach()) and torch.equal(out_nr, out.detach()) and not out_nr.requires_grad
    gout = torch.from_numpy(case.gout).cuda()
    want = _stage_want(case, ref, q_inside)
    for n in (1, 2):                                     # backward(retain_graph=True) twice: twice the gradient
        out.backward(gout, retain_graph=True)
        got = [x.grad.cpu().numpy()] + [w.grad.cpu().numpy() for w in ws]
        for i, (a, b) in enumerate(zip(got, want[1:])):
            assert np.array_equal(a, n * b), (n, i)
    assert np.array_equal(out.detach().cpu().numpy(), want[0])


# -------------------------------------------------------------------------------------------------------------- 5. the clamp
CLAMP_ENTRIES = [(c, e) for c in fa.CLAMP_CASES for e in fa.entries_of(c)]


@pytest.mark.parametrize("case,entry", CLAMP_ENTRIES, ids=["%s-%s" % (c.name, e) for c, e in CLAMP_ENTRIES])
def test_interval_4_kernels_on_pixels_outside_0_255_stay_inside_their_buffers(case, entry):
    """A handful of pixels of x are -300, -1, -0.5, 255.5, 256, 1e9, +-inf and NaN (corners included), and a 4 x 4 block mixes 255
    with NaN of both signs and negative denormals, so that single passes read the anchor at MSB 15 next to sign-set LSBs.  The MSB of
    every key is clamped and the keys are ranked on |LSB| (ft_pass_setup, mulut_ft.h; for every such mix the rows and slots are held
    inside the table on the host, tests/test_ft_abi_cpu.py), so nothing outside a buffer is read or written: the arena's slack is
    untouched, sites that read no such pixel have the reference's bytes in out and inside, and with grad_out zero at the sites that
    do, grad_x is the reference's everywhere and grad_wq wherever no NaN weight was added."""
    lib = _lib()
    case, ref = fa.built(case)
    x, hit, _ = fa.poisoned(case)
    u = case.u
    hit_out = np.repeat(np.repeat(hit, u, axis=2), u, axis=3)
    out, bits, outside = run_forward(lib, case, ref, entry, 4, x=x)
    bad = ["forward: " + b for b in outside]
    want = ref.out.astype(np.float32)
    if not np.array_equal(out[~hit_out], want[~hit_out]):
        bad.append("out differs at %d sites that read no bad pixel" % int((out != want)[~hit_out].sum()))
    if bits is not None and not np.array_equal(bits[~hit], ref.inside[~hit]):
        bad.append("inside differs at %d sites that read no bad pixel" % int((bits != ref.inside)[~hit].sum()))
    quiet = copy.copy(case)
    quiet.gout = np.where(hit_out, np.float32(0), case.gout)
    with fw.wide_oracle():
        ref0 = fx.reference(quiet, check_reach=False)
    gx, gw, outside = run_backward(lib, case, ref, entry, 4, x=x, gout=quiet.gout)
    bad += ["backward: " + b for b in outside]
    bad.append(fx.describe(case, "grad_x", gx, ref0.gx_num))
    for m in range(case.M):
        want = fa.as_f32(ref0.gw_num[m], case.q)
        ok = ~np.isnan(gw[m])
        assert ok.mean() > 0.8, (m, ok.mean())
        if not np.array_equal(gw[m][ok], want[ok]):
            bad.append("grad_wq[%d] differs in %d elements that hold no NaN" % (m, int((gw[m] != want)[ok].sum())))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)
