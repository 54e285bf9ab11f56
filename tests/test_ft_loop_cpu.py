"""Conditions on the cases of tests/ft_loop_cases.py, checked on the reference alone (no GPU): the float64 Adam and the schedule
restated there are torch's, and every case reaches what test_gpu_ft_loop.py needs it to reach."""
import functools

import numpy as np
import pytest
import torch

import ft_loop_cases as L


# ------------------------------------------------------------------------------------------------------------ Adam, schedule
@pytest.mark.parametrize("name", ["A", "B", "D"])      # no weight decay / decay with the lr1 < 0 form / decay with the lr1 >= 0 form
def test_adam_and_schedule_restated_are_torchs_in_float64(name):
    """8 steps of torch.optim.Adam(foreach=False, fused=False) + LambdaLR on float64 CPU tensors, stepped as the reference's loop
    steps them (optimiser, then scheduler), against lr_at and against adam_step from the state torch held before each step: equal up
    to float64 rounding (the restatement forms its products in another order)."""
    case = L.CASES[name]._replace(K=8)
    rng = np.random.default_rng(ord(name))
    p0 = rng.uniform(-1, 1, 4000)
    p0[:10] = 0.0
    grads = [rng.standard_normal(4000) * 10.0 ** rng.uniform(-9, -3, 4000) for _ in range(8)]
    grads[3][:100] = 0.0                                                   # elements without gradient: decay and momentum alone
    t = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([t], lr=case.lr0, betas=(0.9, 0.999), eps=1e-8, weight_decay=case.wd, amsgrad=False, foreach=False, fused=False)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: L.lf(case, x))
    for i in range(1, 9):
        lr = opt.param_groups[0]["lr"]
        assert lr == pytest.approx(L.lr_at(case, i), rel=1e-15, abs=0.0), i
        # the explicit-state helper the GPU file measures its bar with is the same optimiser: from torch's own state, torch's own result
        before = (t.detach().numpy().copy(),) + ((opt.state[t]["exp_avg"].numpy().copy(), opt.state[t]["exp_avg_sq"].numpy().copy()) if i > 1
                                                  else (np.zeros(4000), np.zeros(4000)))
        t.grad = torch.tensor(grads[i - 1], dtype=torch.float64)
        opt.step()
        sched.step()
        tp, tm, tv, ts = L.torch_adam_step(before[0], grads[i - 1], before[1], before[2], i - 1, lr, case.wd, torch.float64)
        assert np.array_equal(tp, t.detach().numpy()) and np.array_equal(tv, opt.state[t]["exp_avg_sq"].numpy()) and ts == i
        # the restatement, one step from torch's own state.  Bars: a handful of roundings of 1.1e-16 relative to the operands -- NOT to the
        # result, exp_avg + 0.1 (g - exp_avg) cancels; an error d in exp_avg reaches p as (lr / bc1) d / denom, where bc1 >= 0.1 and
        # denom >= 0.35 |g| (exp_avg_sq holds 0.001 g^2 of this step and bc2 <= 0.008 over 8 steps): below 1e-13 lr
        p, m, v, step = L.adam_step(before[0], grads[i - 1], before[1], before[2], i - 1, lr, case.wd)
        st = opt.state[t]
        g = grads[i - 1] + case.wd * before[0]
        for got, want, tol, what in ((p, t.detach().numpy(), 1e-15 * np.abs(before[0]) + 1e-13 * lr, "p"),
                                     (m, st["exp_avg"].numpy(), 1e-15 * (np.abs(before[1]) + np.abs(g)), "exp_avg"),
                                     (v, st["exp_avg_sq"].numpy(), 1e-15 * (before[2] + g * g), "exp_avg_sq")):
            assert (np.abs(got - want) <= tol).all(), (what, i, float((np.abs(got - want) - tol).max()))
        assert step == int(st["step"].item())
    assert L.lr_at(case, 1) == case.lr0                                    # lf(0) = 1 in both forms
    end = 0.2 if case.lr1 < 0 else case.lr1 / case.lr0
    assert L.lf(case, case.K) == pytest.approx(end, rel=1e-12)             # and the form's floor at totalIter


def test_weight_decay_is_l2_in_the_gradient():
    p, m, v, s = L.adam_step(np.array([0.5]), np.array([0.0]), np.zeros(1), np.zeros(1), 0, 1e-2, 1e-2)
    assert m[0] == pytest.approx(0.1 * 0.5e-2) and p[0] == pytest.approx(0.5 - 1e-2 * 0.5e-2 / (0.5e-2 + 1e-8))
    p, m, v, s = L.adam_step(np.array([0.5]), np.array([0.0]), np.zeros(1), np.zeros(1), 0, 1e-2, 0.0)
    assert p[0] == 0.5 and m[0] == 0.0


def test_adam_entry_point_refuses_before_the_device_is_touched():
    """mulut_ft_adam of include/mulut.h: NULL lists and elements, T < 1, n[t] < 1, step < 1, a beta outside [0, 1) -> MULUT_EINVAL (no GPU here)"""
    import ctypes
    from mulut_amd import _native
    lib = _native.load()
    bufs = [ctypes.create_string_buffer(16) for _ in range(8)]       # never dereferenced
    ptrs = lambda k, hole=None: (ctypes.c_void_p * 2)(*[None if j == hole else ctypes.addressof(bufs[2 * k + j]) for j in range(2)])      # noqa: E731
    n = lambda *v: (ctypes.c_longlong * 2)(*v)      # noqa: E731
    ok = dict(p=ptrs(0), g=ptrs(1), m=ptrs(2), v=ptrs(3), n=n(4, 4), T=2, step=1, b1=0.9, b2=0.999)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mulut_ft_adam(0, a["p"], a["g"], a["m"], a["v"], a["n"], a["T"], a["step"], 1e-3, a["b1"], a["b2"], 1e-8, 0.0, None)

    for kw in [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=None), dict(T=0), dict(T=-1), dict(step=0), dict(n=n(4, 0)), dict(n=n(-1, 4)),
               dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan")), dict(p=ptrs(0, 1)), dict(g=ptrs(1, 0)), dict(m=ptrs(2, 1)), dict(v=ptrs(3, 0))]:
        assert call(**kw) == -1, kw
    assert "mulut_ft_adam" in _native.EXPORTS


def test_bytes_survive_the_float32_round_trip():
    """x and the target are k / 255 in float32; the forward's * 255 gives k back exactly in float32 (and not in float64: why the
    oracle's quant_f32 scales its input in float32)"""
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal((k / np.float32(255)) * np.float32(255), k)
    assert not np.array_equal((k / np.float32(255)).astype(np.float64) * 255.0, k.astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ free run
@functools.lru_cache(maxsize=None)
def free_run(name):
    """The reference's loop on the float32 oracle: unfused float32 Adam + LambdaLR over the case's K batches.  Per step: the weights
    and Adam state before it, the oracle's Step, the learning rate; and the final weights."""
    case = L.CASES[name]
    params = {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in L.start_weights(case).items()}
    opt = torch.optim.Adam(list(params.values()), lr=case.lr0, betas=(0.9, 0.999), eps=1e-8, weight_decay=case.wd, amsgrad=False,
                           foreach=False, fused=False)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: L.lf(case, x))
    steps = []
    for im, lb in L.batches(case):
        w = {k: p.detach().numpy().copy() for k, p in params.items()}
        state = {k: ((opt.state[p]["exp_avg"].numpy().copy(), opt.state[p]["exp_avg_sq"].numpy().copy(), int(opt.state[p]["step"].item()))
                     if p in opt.state else (np.zeros_like(w[k]), np.zeros_like(w[k]), 0)) for k, p in params.items()}
        r = L.oracle_step(case, w, im, lb, torch.float32)
        for k, p in params.items():
            p.grad = torch.from_numpy(r.grads[k].copy())
        steps.append((w, state, r, opt.param_groups[0]["lr"], im, lb))
        opt.step()
        sched.step()
    return steps, {k: p.detach().numpy().copy() for k, p in params.items()}


@pytest.mark.parametrize("name", list(L.CASES))
def test_case_reaches_what_it_is_for(name):
    case = L.CASES[name]
    steps, final = free_run(name)
    assert len(steps) == case.K
    ws = [s[0] for s in steps] + [final]
    qs = [L.quantised(w) for w in ws]
    beyond_moving, pushed = 0, 0
    for key in L.keys(case):
        # a quantised entry of every table changes between two steps: a stale quantised table would show
        changed = [int((qs[i][key] != qs[i + 1][key]).sum()) for i in range(case.K)]
        assert sum(c > 0 for c in changed[:-1]) >= 1, (key, changed)       # (before the last step: a later forward sees it)
        for i, (w, state, r, lr, im, lb) in enumerate(steps):
            g = r.grads[key]
            assert np.count_nonzero(g) > 0, (key, i)                       # no batch is empty of gradient for any table
            assert not g[r.beyond[key]].any()                              # the oracle stops the gradient beyond the clamp
            # entries beyond the quantiser's clamp, |round(w * 127)| > 127: their gradient is stopped and the step moves them all the same
            # (momentum, weight decay); `pushed`: those of them that the loop itself took there, inside the clamp at the start
            moving = r.beyond[key] & (ws[i + 1][key] != w[key])
            beyond_moving += int(moving.sum())
            pushed += int((moving & ~steps[0][2].beyond[key]).sum())
    assert beyond_moving >= 1, "no entry beyond the quantiser's clamp keeps moving"
    for i, (w, state, r, lr, im, lb) in enumerate(steps):
        inside = (r.pred >= 0) & (r.pred <= 255)
        assert 0 < inside.sum() < inside.size, (i, int(inside.sum()), inside.size)      # the final clamp passes and stops gradient
    print(name, "entries beyond the quantiser's clamp and moving, summed over steps: %d, of them pushed there by the loop: %d" % (beyond_moving, pushed))


def test_batches_and_tables_are_as_described():
    for case in L.CASES.values():
        bs = L.batches(case)
        assert len(bs) == case.K
        for im, lb in bs:
            assert im.shape == (case.batch, 1, case.crop, case.crop) and lb.shape == (case.batch, 1, case.crop * case.scale, case.crop * case.scale)
            assert im.dtype == lb.dtype == np.float32
        rows = 2 ** (8 - case.interval) + 1
        for key, t in L.start_tables(case).items():
            assert t.dtype == np.int8 and t.shape == (rows ** 4, case.scale ** 2 if key.startswith("s%d_" % case.stages) else 1)
            assert [int(t[r, 0]) for r, _ in L.forced_rows(case)] == [v for _, v in L.forced_rows(case)]
        assert sorted(L.start_tables(case)) == sorted(L.keys(case))


def test_loss_bar_is_what_float32_costs_on_the_oracles_own_output():
    import torch.nn.functional as F
    worst, where = 0.0, None
    for name, case in L.CASES.items():
        for i, (w, state, r32, lr, im, lb) in enumerate(free_run(name)[0]):
            r64 = L.oracle_step(case, w, im, lb, torch.float64)
            l32 = float(F.mse_loss(r64.out_t.to(torch.float32), torch.from_numpy(lb)).item())
            rel = abs(l32 - r64.loss) / r64.loss
            worst, where = max((worst, where), (rel, (name, i + 1)))
    print("largest |mse32 - mse64| / mse64: %.3g at %s; LOSS_F32_REL = %.3g" % (worst, where, L.LOSS_F32_REL))
    assert L.LOSS_F32_REL / 2 < worst <= L.LOSS_F32_REL


# ------------------------------------------------------------------------------------------- why one step from a common state
def test_float32_and_float64_oracles_part_by_full_adam_steps_and_why():
    """The observation behind the design, over case A: from the same weights and Adam state, the float32 oracle and oracle.ft_torch
    run in float64 as it stands, each fed its own gradient, give updates that differ by more than lr / 2 (a step is at most about lr)
    on some table elements.  Recorded: the count; asserted: that it is not zero.

    What the count is NOT is Adam turning rounding noise into steps.  The float64 run's x * 255 is not integer-valued (k / 255 is a
    float32 value), so its LSBs carry fractions of 1e-6, ties between keys break the other way, sites land in other simplices and a
    sixth of its output BYTES differ: another function, not another rounding.  With the input scaled and the tables quantised in
    float32 (quant_f32) the float64 oracle gives the float32 oracle's bytes and no update differs by lr / 2 -- the largest difference
    is printed (measured: 4e-4 lr; eps = 1e-8 of Adam is far above the gradients' float32 noise of about 1e-11)."""
    import torch.nn.functional as F
    from oracle import ft_torch
    case = L.CASES["A"]
    steps, _ = free_run("A")
    count, count_q, worst_q, bytes_off, total = 0, 0, 0.0, 0, 0
    for w, state, r32, lr, im, lb in steps:
        r64 = L.oracle_step(case, w, im, lb, torch.float64)
        assert np.array_equal(r64.out, r32.out)                            # quant_f32: the same bytes
        tw = {k: torch.from_numpy(v).to(torch.float64).requires_grad_(True) for k, v in w.items()}
        out = ft_torch.forward(tw, torch.from_numpy(im).to(torch.float64), case.stages, case.modes, case.scale, case.interval)
        F.mse_loss(out, torch.from_numpy(lb).to(torch.float64)).backward()
        bytes_off += int((np.rint(out.detach().numpy() * 255.0) != r32.out).sum())
        for key in L.keys(case):
            m, v, step = state[key]
            p32 = L.adam_step(w[key], r32.grads[key], m, v, step, lr, case.wd)[0]
            p64 = L.adam_step(w[key], tw[key].grad.numpy(), m, v, step, lr, case.wd)[0]
            p64q = L.adam_step(w[key], r64.grads[key], m, v, step, lr, case.wd)[0]
            count += int((np.abs(p32 - p64) > lr / 2).sum())
            count_q += int((np.abs(p32 - p64q) > lr / 2).sum())
            worst_q = max(worst_q, float(np.abs(p32 - p64q).max()) / lr)
            total += int(np.count_nonzero(r64.grads[key]))
    print("updates differing by more than lr / 2 from the float32 oracle's, over %d steps and %d elements with gradient: plain float64 %d "
          "(%d output bytes differ), quant_f32 float64 %d (largest difference %.2g lr)" % (case.K, total, count, bytes_off, count_q, worst_q))
    assert count > 0 and bytes_off > 0
    assert count_q == 0
