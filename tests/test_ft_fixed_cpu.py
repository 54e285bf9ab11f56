"""The bit-reproducible (fixed-point) backward of a fine-tune stage on the CPU:
  * the host model (tests/host_emul/ft_exact_host.cpp: mulut_ft_exact.h walked with plain int64 adds) against oracle/ft_torch.py's
    autograd on every case of tests/ft_fixed_cases.py, at the bar tests/ft_grad_bar.py holds the float kernels to;
  * the model's bytes do not depend on the order in which the sites are walked;
  * the headroom cases end without the model's abort, and reach the accumulator the derivation of the scale says they reach;
  * mulut_ft_exact_stage_backward and mulut_ft_exact_ws_bytes refuse what they must, before any device is touched.
(The host-layer traces, tests/golden/host_abi_trace.txt and host_tables_trace.txt, are held by test_host_abi_cpu.py and
test_host_tables_cpu.py, which link every file of _native.SOURCES: the new one is in that list.)"""
import ctypes
import os

import numpy as np
import pytest
import torch

import ft_fixed_cases as fc
import ft_grad_bar
import ft_wide_cases as fw
from conftest import ROOT


def oracle_grads(case):
    """d/d tables and d/d x of sum(pred * g), g = mask * grad_out / avg (the clamp's backward, then d(pred / avg)), by the oracle's
    autograd.  The oracle runs in float64 on the case's float32 values: the bar is for the model, and a float32 oracle's own sums (up to
    36,864 equal terms into one element in the headroom cases) would spend it."""
    case.build()
    tabs = [torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in case.tables]
    x = torch.from_numpy(case.x.astype(np.float64)).requires_grad_(True)
    g = (case.gout / np.float32(case.avg)).astype(np.float64) * case.mask_hr()
    with fw.wide_oracle() as ft:
        _, pred = ft.stage(tabs, x, case.modes, bool(case.last), case.u, case.interval, quantised=True)
        pred.backward(torch.from_numpy(g))
    return np.stack([t.grad.numpy() for t in tabs]), x.grad.numpy()


@pytest.mark.parametrize("case", fc.CASES + [fc.E7], ids=lambda c: c.name)
def test_model_is_inside_the_float_kernels_bar_and_order_free(case):
    try:
        want_w, want_x = oracle_grads(case)
        got = fc.expected(case)
        print(case.name, "S_w %d S_x %d, largest sums 2^%.2f (tables) 2^%.2f (input)" % (got.Sw, got.Sx, np.log2(max(got.max_w, 1)), np.log2(max(got.max_x, 1))))
        assert np.abs(want_x).max() > 0 and np.abs(want_w).max() > 0
        ft_grad_bar.close(got.gx.astype(np.float64), want_x, case.name + " grad_x")
        for m in range(case.M):
            ft_grad_bar.close(got.gw[m].astype(np.float64), want_w[m], case.name + " grad_wq[%d]" % m)
        for order in ("descending", "shuffled"):
            other = fc.expected(case, order=order, seed=7)
            assert np.array_equal(other.gw.view(np.uint32), got.gw.view(np.uint32)), order
            assert np.array_equal(other.gx.view(np.uint32), got.gx.view(np.uint32)), order
            assert (other.Sw, other.Sx) == (got.Sw, got.Sx)      # (the largest PARTIAL sum on the way may differ: only the sums are order-free)
    finally:
        case.free()


@pytest.mark.parametrize("case", fc.HEADROOM, ids=lambda c: c.name)
def test_headroom_cases_use_what_the_derivation_says(case):
    """4 x 1 x 48 x 48 sites of a constant image, one mode, avg 1, every grad_out = gmax just below 2: the anchor row gets weight q / q
    from every site under every rotation, 36,864 contributions of llrint(gmax 2^S_w) each.  S_w = 61 - 1 - 16: the sum is
    36,864 (2^45 - 2^21) = 2^60.17 of the 2^62 no accumulator may leave."""
    try:
        got = fc.expected(case)
        nsite = int(np.prod(case.shape))
        assert got.gbits == int(np.float32(case.gmax).view(np.uint32)) and got.Sw == 61 - 1 - 16
        unit = int(float(case.gmax) * 2.0 ** got.Sw)
        assert unit == 2 ** 45 - 2 ** 21
        assert got.max_w == 4 * nsite * unit and 2 ** 60 < got.max_w < 2 ** 62
        assert 0 < got.max_x < 2 ** 62
        print(case.name, "tables 2^%.3f, input 2^%.3f (S_x %d)" % (np.log2(got.max_w), np.log2(got.max_x), got.Sx))
        # the anchor row of the constant image holds the whole sum: 36,864 gmax, exactly representable steps of the result
        row = (128 >> 4) * (17 ** 3 + 17 ** 2 + 17 + 1)
        assert np.all(got.gw[0][row] == np.float32(case.sign * 4.0 * nsite * float(case.gmax)))
    finally:
        case.free()


# ------------------------------------------------------------------------------------------------------------------- refusals
EINVAL, EMODE, EUNSUPPORTED, ENODEVICE, EWORKSPACE = -1, -2, -5, -7, -9


def _call(lib, interval=5, modes=b"sdy", u=4, x=1, mask=1, gout=1, gw=1, gx=1, tab0=1, B=1, C=1, H=4, W=4, ws=1, ws_bytes=None, misalign=0):
    """The entry point with dummy non-null addresses: every refusal tested here is decided before a pointer is followed."""
    M = len(modes) if modes is not None else 1
    buf = np.zeros(4096, np.float32)
    p = lambda on: ctypes.c_void_p(buf.ctypes.data if on else None)      # noqa: E731
    n = max(min(M, 8), 1)
    ptrs = (ctypes.c_void_p * n)(*[buf.ctypes.data] * n)
    tabs = (ctypes.c_void_p * n)(*[buf.ctypes.data if (tab0 or i) else None for i in range(n)])
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return lib.mulut_ft_exact_stage_backward(0, interval, tabs, modes, 1, u, p(x), p(gout), p(mask), B, C, H, W, ptrs if gw else None, p(gx),
                                             ctypes.c_void_p(buf.ctypes.data + misalign if ws else None), ws_bytes, None)


def test_exports_are_declared_listed_and_built():
    from mulut_amd import _native
    header = open(os.path.join(ROOT, "include", "mulut.h")).read()
    for name in ("mulut_ft_exact_ws_bytes", "mulut_ft_exact_stage_backward"):
        assert name in _native.EXPORTS and name + "(" in header
        assert hasattr(_native.load(), name)
    assert "mulut_ft_exact.hip" in _native.SOURCES and "mulut_ft_exact.h" in _native.HEADERS      # built, hashed, and linked by the host-ABI harness
    assert "sr/model.py:69-312" in header[header.index("BIT-REPRODUCIBLE"):header.index("long long mulut_ft_exact_ws_bytes")]


def test_entry_point_refuses_before_touching_a_device():
    from mulut_amd import _native
    lib = _native.load()
    # the order of mulut_ft_wide_stage_backward: the family's early pointer, then ft_fill()
    assert _call(lib, gw=0, interval=9, modes=b"q") == EINVAL
    assert _call(lib, x=0, interval=9) == EINVAL
    assert _call(lib, modes=None) == EINVAL
    assert _call(lib, mask=0) == EINVAL
    for kw in (dict(B=0), dict(C=-1), dict(H=0), dict(W=-3)):
        assert _call(lib, **kw) == EINVAL
    assert _call(lib, interval=3, modes=b"q") == EUNSUPPORTED
    assert _call(lib, interval=7) == EUNSUPPORTED
    assert _call(lib, u=0, modes=b"q") == EUNSUPPORTED
    assert _call(lib, u=5) == EUNSUPPORTED
    assert _call(lib, modes=b"") == EUNSUPPORTED
    assert _call(lib, modes=b"sdysdysdy") == EUNSUPPORTED
    for m in (b"x", b"sdq", b"ehoS"):
        assert _call(lib, modes=m, gout=0) == EMODE
    assert _call(lib, tab0=0, gout=0) == EINVAL
    # then the call's own pointers, the size, the workspace
    assert _call(lib, gout=0, ws=0) == EINVAL
    assert _call(lib, gx=0, ws=0) == EINVAL
    assert _call(lib, B=1 << 16, C=1 << 15, H=1, W=1, ws=0) == EUNSUPPORTED      # 2^31 sites
    assert _call(lib, B=1 << 30, C=1 << 30, H=1 << 30, W=1 << 30, ws=0) == EUNSUPPORTED
    assert _call(lib, ws=0, ws_bytes=0) == EINVAL
    assert _call(lib, misalign=4, ws_bytes=0) == EINVAL
    for interval in (4, 5, 6):
        for modes, u in ((b"sdy", 1), (b"eho", 4), (b"sdyehosd", 3)):
            need = lib.mulut_ft_exact_ws_bytes(interval, modes, u, 2, 3, 5, 7)
            assert need == 8 * (1 + len(modes) * fc.rows_of(interval) * u * u + 2 * 3 * 5 * 7)
            kw = dict(interval=interval, modes=modes, u=u, B=2, C=3, H=5, W=7)
            assert _call(lib, ws_bytes=need - 1, **kw) == EWORKSPACE
            assert _call(lib, ws_bytes=0, **kw) == EWORKSPACE
            assert _call(lib, ws_bytes=-5, **kw) == EWORKSPACE
            if not torch.cuda.is_available():
                assert _call(lib, ws_bytes=need, **kw) == ENODEVICE      # well-formed: only the device is missing (no CPU path)


def test_ws_bytes_refuses_what_the_call_refuses():
    from mulut_amd import _native
    q = _native.load().mulut_ft_exact_ws_bytes
    assert q(4, None, 1, 1, 1, 4, 4) == EINVAL
    assert q(4, b"sdy", 1, 0, 1, 4, 4) == EINVAL and q(4, b"sdy", 1, 1, 1, 4, -1) == EINVAL
    assert q(3, b"sdy", 1, 1, 1, 4, 4) == EUNSUPPORTED and q(7, b"sdy", 1, 1, 1, 4, 4) == EUNSUPPORTED
    assert q(4, b"sdy", 0, 1, 1, 4, 4) == EUNSUPPORTED and q(4, b"sdy", 5, 1, 1, 4, 4) == EUNSUPPORTED
    assert q(4, b"", 1, 1, 1, 4, 4) == EUNSUPPORTED and q(4, b"sdyehosdy", 1, 1, 1, 4, 4) == EUNSUPPORTED
    assert q(4, b"sdx", 1, 1, 1, 4, 4) == EMODE
    assert q(4, b"s", 1, 1 << 16, 1 << 15, 1, 1) == EUNSUPPORTED
    assert q(4, b"s", 1, (1 << 31) - 1, 1, 1, 1) == 8 * (1 + 83521 + (1 << 31) - 1)
    assert q(6, b"sdyeho", 4, 256, 1, 48, 48) == 8 * (1 + 6 * 625 * 16 + 256 * 48 * 48)


def test_module_and_driver_take_the_switch_without_a_device(tmp_path):
    from mulut_amd import finetune, finetune_lut
    for m in "sd":
        np.save(tmp_path / ("LUT_x2_6bit_int8_s1_%s.npy" % m), np.zeros((625, 4), np.int8))
    for cls, interval in ((finetune.MuLUTInterval, 6), (finetune.MuLUTWide, 6)):
        assert cls(str(tmp_path), 1, "sd", upscale=2, interval=interval).deterministic is False
        assert cls(str(tmp_path), 1, "sd", upscale=2, interval=interval, deterministic=True).deterministic is True
    opt = finetune_lut.build_parser().parse_args(["-e", "x"])
    assert opt.deterministic is False and opt.seed is None
    opt = finetune_lut.build_parser().parse_args(["-e", "x", "--deterministic"])
    assert opt.deterministic is True and opt.seed is None      # allowed: reproducible only if the caller fixes the seed
    assert "--seed" in finetune_lut.build_parser().format_help().split("--deterministic")[-1][:600]      # the flag's help says so
