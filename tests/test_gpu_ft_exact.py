"""The fine-tune stage kernels against exact integer references, and the quantiser kernels against torch, bit for bit.

The float bars of test_gpu_finetune.py / test_gpu_ft_interval.py (norm-wise 2e-5 of the largest element) are honest about float
reordering and blind to one lost, doubled or misplaced term of a rarely-touched row -- what an unflushed cache entry, a lost
eviction or a band slot off by one at the rim produces.  In the cases of tests/ft_exact_cases.py every term is an integer over q
and every sum stays below 2^24 / q, so float32 sums are exact in any order (premise: tests/test_ft_exact_cpu.py) and the kernels
must give the reference's bytes: out, the clamp mask `inside`, grad_x and every grad_wq, at any batch size, on every run.
No tolerance anywhere in this file's exact tests."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ft_exact_cases as fx      # noqa: E402

pytestmark = pytest.mark.gpu


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _stage_on_gpu(lib, case, wq, x, gout, masked, inside=None):
    """One forward (when `inside` is None) or one backward through the C ABI.  Interval 4: the recomputing pair or, `masked`, the
    _mask pair; intervals 5 and 6 have the mask pair only."""
    B, C, H, W = case.shape
    u, iv, modes, last = case.u, case.interval, case.modes.encode(), case.last
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if inside is None:
        out = torch.full((B, C, H * u, W * u), float("nan"), dtype=torch.float32, device="cuda")
        mask = torch.full(case.shape, -1, dtype=torch.int16, device="cuda")
        if iv != 4:
            rc = lib.mulut_ft_interval_stage_forward(0, iv, _ptrs(wq), modes, last, u, x.data_ptr(), B, C, H, W, out.data_ptr(), mask.data_ptr(), st)
        elif masked:
            rc = lib.mulut_ft_stage_forward_mask(0, _ptrs(wq), modes, last, u, x.data_ptr(), B, C, H, W, out.data_ptr(), mask.data_ptr(), st)
        else:
            rc = lib.mulut_ft_stage_forward(0, _ptrs(wq), modes, last, u, x.data_ptr(), B, C, H, W, out.data_ptr(), st)
        assert rc == 0, rc
        return out.cpu().numpy(), mask.cpu().numpy().view(np.uint16)
    gw = [torch.zeros_like(w) for w in wq]
    gx = torch.zeros_like(x)
    if iv != 4:
        rc = lib.mulut_ft_interval_stage_backward(0, iv, _ptrs(wq), modes, last, u, x.data_ptr(), gout.data_ptr(), inside.data_ptr(), B, C, H, W,
                                                  _ptrs(gw), gx.data_ptr(), st)
    elif masked:
        rc = lib.mulut_ft_stage_backward_mask(0, _ptrs(wq), modes, last, u, x.data_ptr(), gout.data_ptr(), inside.data_ptr(), B, C, H, W,
                                              _ptrs(gw), gx.data_ptr(), st)
    else:
        rc = lib.mulut_ft_stage_backward(0, _ptrs(wq), modes, last, u, x.data_ptr(), gout.data_ptr(), B, C, H, W, _ptrs(gw), gx.data_ptr(), st)
    assert rc == 0, rc
    return gx.cpu().numpy(), [g.cpu().numpy() for g in gw]


@pytest.mark.parametrize("case", fx.CASES, ids=lambda c: c.name)
def test_stage_kernels_equal_the_integer_reference(case):
    from mulut_amd import _native
    lib = _native.load()
    case.build()
    try:
        ref = fx.reference(case)      # asserts the exactness cap and the case's reach
        wq = [torch.from_numpy(t.astype(np.float32)).cuda() for t in case.tables]
        x, gout = torch.from_numpy(case.x).cuda(), torch.from_numpy(case.gout).cuda()
    finally:
        case.tables = case.x = case.gout = None
    print(case.name, "sum |terms| * q =", ref.cap, ref.reach)
    bad = []
    forms = (False, True) if case.interval == 4 else (True,)
    inside = None
    for masked in forms:
        form = "mask pair" if masked else "recomputing pair"
        out, mask = _stage_on_gpu(lib, case, wq, x, gout, masked)
        bad.append(fx.describe(case, "out (%s)" % form, out, ref.out, q=1))
        if masked:
            bits = mask & np.uint16((1 << case.u * case.u) - 1)
            bad.append(fx.describe(case, "inside, bits 0..u*u-1 (1/q = one mask value)", bits.astype(np.float32), ref.inside.astype(np.int64), q=1))
            inside = torch.from_numpy(mask.view(np.int16)).cuda()
    for masked in forms:
        form = "mask pair" if masked else "recomputing pair"
        runs = [_stage_on_gpu(lib, case, wq, x, gout, masked, inside) for _ in range(2)]
        gx, gw = runs[0]
        bad.append(fx.describe(case, "grad_x (%s)" % form, gx, ref.gx_num))
        for m in range(case.M):
            bad.append(fx.describe(case, "grad_wq[%d] (%s)" % (m, form), gw[m], ref.gw_num[m]))
        # with exact sums the order of the atomics is immaterial: a second run must give the same bytes (a failure here and not
        # above would be impossible; one here AND above reads as "nondeterministic", one above alone as "systematically wrong")
        for a, b, what in zip([runs[0][0]] + runs[0][1], [runs[1][0]] + runs[1][1], ["grad_x"] + ["grad_wq[%d]" % m for m in range(case.M)]):
            if not np.array_equal(a, b):
                bad.append("%s: %s (%s) differs between two runs of one backward in %d elements" % (case.name, what, form, int((a != b).sum())))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------ quantiser
def halfway_weights():
    """every float32 w with fl(w * 127f) == k + 0.5 exactly, k in -129..128, searched among the neighbours of (k + 0.5) / 127"""
    found = {}
    for k in range(-129, 129):
        c = np.float32((k + 0.5) / 127.0)
        cand = [c]
        for direction in (-np.inf, np.inf):
            w = c
            for _ in range(8):
                w = np.nextafter(w, np.float32(direction))
                cand.append(w)
        cand = np.array(cand, np.float32)
        hit = cand[cand * np.float32(127.0) == np.float32(k + 0.5)]
        if len(hit):
            found[k] = hit
    return found


def quantiser_weights(M, n, seed):
    rng = np.random.default_rng(seed)
    ties = halfway_weights()
    one, big = np.float32(1.0), np.float32(127.5 / 127.0)
    special = np.concatenate([np.concatenate(list(ties.values())), np.array([
        1.0, -1.0, np.nextafter(one, np.float32(np.inf)), np.nextafter(-one, np.float32(-np.inf)), np.nextafter(one, np.float32(0)),
        np.nextafter(-one, np.float32(0)), big, np.nextafter(big, np.float32(np.inf)), np.nextafter(big, np.float32(0)), -big,
        np.nextafter(-big, np.float32(-np.inf)), np.nextafter(-big, np.float32(0)), 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1e30, -1e30,
        np.inf, -np.inf, np.nan, -np.nan], np.float32)])
    total = M * n
    jitter = ((rng.integers(-140, 141, total) + rng.uniform(-0.5, 0.5, total)) / 127.0).astype(np.float32)      # (k + delta) / 127, |w| > 1 included
    flat = np.concatenate([np.roll(special, seed)[:total], jitter])[:total] if total <= len(special) else \
        rng.permutation(np.concatenate([special, jitter[len(special):]]))
    return flat.reshape(M, n)


def same_bits(got, want):
    """== plus equal NaN positions (the sign of zero is not compared)"""
    return bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


def test_halfway_ties_exist_for_even_and_odd_k_on_both_sides_of_zero():
    ties = halfway_weights()
    for sign in (-1, 1):
        for parity in (0, 1):
            ks = [k for k in ties if (k + 0.5) * sign > 0 and k % 2 == parity and abs(k + 0.5) < 127]
            assert len(ks) >= 10, (sign, parity, ks)
    assert 127 in ties and -128 in ties      # +-127.5: round-half-even gives +-128, outside the clamp


@pytest.mark.parametrize("n", [1, 255, 257, 625 * 9, 6561 * 16, 83521 * 16])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_quantiser_kernels_equal_torch_bit_for_bit(M, n):
    from mulut_amd import _native
    lib = _native.load()
    w = quantiser_weights(M, n, 1000 * M + n % 997)
    g = np.random.default_rng(n + M).standard_normal((M, n)).astype(np.float32)
    wt, gt = torch.from_numpy(w), torch.from_numpy(g)
    r = torch.round(wt * 127)
    want_fwd = torch.clamp(r, -127, 127).numpy()
    want_bwd = (gt * ((r >= -127) & (r <= 127)) * 127).numpy()
    if M * n > 1000:
        assert np.isnan(w).any() and np.isinf(w).any() and (np.abs(w) > 1).any()
        assert np.isnan(want_fwd[np.isnan(w)]).all() and (want_bwd[np.isnan(w)] == 0).all()      # what torch does with NaN
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = [wt[m].cuda() for m in range(M)]
    outs = [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(M)]
    grads = [gt[m].cuda() for m in range(M)]
    assert lib.mulut_ft_quantize(0, _ptrs(ws), _ptrs(outs), M, n, st) == 0
    assert lib.mulut_ft_quantize_backward(0, _ptrs(ws), _ptrs(grads), M, n, st) == 0      # in place on the gradient
    for m in range(M):
        got_f, got_b = outs[m].cpu().numpy(), grads[m].cpu().numpy()
        for what, got, want in (("forward", got_f, want_fwd[m]), ("backward", got_b, want_bwd[m])):
            if not same_bits(got, want):
                i = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
                raise AssertionError("quantiser %s, table %d: %d of %d differ; first: %s" % (
                    what, m, len(i), n, [(int(j), float(w[m][j]), float(got[j]), float(want[j])) for j in i[:8]]))
        assert torch.equal(ws[m].cpu().view(torch.int32), wt[m].view(torch.int32))      # the weights are read only


# ------------------------------------------------------------------------------------------------------- off-grid weights, module level
def _close(g, r, what):
    """the bars of test_more_shapes_vs_cpu_oracle"""
    scale = max(float(np.abs(r).max()), 1e-30)
    assert float(np.abs(g - r).max()) <= 2e-5 * scale, (what, float(np.abs(g - r).max()), scale)
    sig = np.abs(r) > 0.01 * scale
    assert np.allclose(g[sig], r[sig], rtol=5e-5, atol=0.0), what


@pytest.mark.parametrize("interval", [4, 5, 6])
def test_module_with_off_grid_weights_vs_cpu_oracle(tmp_path, interval):
    """After the first optimiser step no weight is k / 127 any more, and some leave [-1, 1], where the quantiser's clamp must stop
    the gradient: the module with such weights against oracle.ft_torch.forward on the same floats."""
    from mulut_amd.finetune import MuLUT, MuLUTInterval
    from oracle import ft_torch
    stages, modes, scale, shape = 2, "sdy", 4, (4, 1, 24, 24)
    rng = np.random.default_rng(40 + interval)
    rows = (2 ** (8 - interval) + 1) ** 4
    keys = ["s%d_%s" % (s + 1, m) for s in range(stages) for m in modes]
    for key in keys:
        vnum = scale * scale if key[1] == str(stages) else 1
        np.save(tmp_path / ("LUT_x%d_%dbit_int8_%s.npy" % (scale, interval, key)), rng.integers(-127, 128, (rows, vnum), dtype=np.int8))
    net = (MuLUT if interval == 4 else MuLUTInterval)(str(tmp_path), stages, modes, upscale=scale, interval=interval).cuda()
    wcpu = {}
    with torch.no_grad():
        for key in keys:
            p = getattr(net, "weight_" + key)
            w = p.cpu().numpy()
            w = (w + rng.uniform(-0.45, 0.45, w.shape).astype(np.float32) / np.float32(127)).astype(np.float32)      # off the grid
            w = np.where(rng.random(w.shape) < 0.05, w * np.float32(1.4), w).astype(np.float32)                       # some beyond +-1
            p.copy_(torch.from_numpy(w))
            wcpu[key] = torch.from_numpy(w.copy()).requires_grad_(True)
    x = rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)
    tgt = rng.random((shape[0], shape[1], shape[2] * scale, shape[3] * scale), dtype=np.float32)
    xc = torch.from_numpy(x).requires_grad_(True)
    yc = ft_torch.forward(wcpu, xc, stages, modes, scale, interval)
    torch.nn.functional.mse_loss(yc, torch.from_numpy(tgt)).backward()
    # which clamped elements the batch touches: the same oracle on the weights brought back to [-1, 1] computes the same forward
    # (the quantised tables are the same), and there the clamp passes the gradient
    wopen = {k: torch.clamp(v.detach(), -1, 1).requires_grad_(True) for k, v in wcpu.items()}
    yo = ft_torch.forward(wopen, torch.from_numpy(x), stages, modes, scale, interval)
    assert torch.equal(yo, yc.detach())
    torch.nn.functional.mse_loss(yo, torch.from_numpy(tgt)).backward()
    xg = torch.from_numpy(x).cuda().requires_grad_(True)
    yg = net(xg)
    torch.nn.functional.mse_loss(yg, torch.from_numpy(tgt).cuda()).backward()
    assert np.abs(yg.detach().cpu().numpy() - yc.detach().numpy()).max() <= 1e-5
    _close(xg.grad.cpu().numpy(), xc.grad.numpy(), "gx")
    touched_clamped = 0
    for key in keys:
        g = getattr(net, "weight_" + key).grad.cpu().numpy()
        _close(g, wcpu[key].grad.numpy(), key)
        clamped = (torch.round(wcpu[key].detach() * 127).abs() > 127).numpy()
        hit = clamped & (wopen[key].grad.numpy() != 0)
        touched_clamped += int(hit.sum())
        assert (wcpu[key].grad.numpy()[clamped] == 0).all()
        assert (g[clamped] == 0).all(), (key, int((g[clamped] != 0).sum()))
    print("interval", interval, "touched table elements beyond the quantiser's clamp:", touched_clamped)
    assert touched_clamped >= 1
