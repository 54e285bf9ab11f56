"""The premise of the exact fine-tune tests (tests/test_gpu_ft_exact.py), checked on the reference alone, and the refusals of the
quantiser entry points.

For every exact case (tests/ft_exact_cases.py) the float32 oracle must equal the float64 oracle exactly -- outputs, pred, grad_x
and every table gradient: the reference a float32 kernel is held to is itself free of any summation order.  reference() asserts,
for both, that every gradient times q is an integer, the exactness cap (sum |terms| * q < 2^24 per table element) and that the
case reaches what it was built for."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ft_exact_cases as fx      # noqa: E402


@pytest.mark.parametrize("case", fx.CASES, ids=lambda c: c.name)
def test_float32_oracle_equals_float64_oracle_exactly(case):
    case.build()
    try:
        r64 = fx.reference(case, torch.float64)
        r32 = fx.reference(case, torch.float32, check_reach=False)
    finally:
        case.tables = case.x = case.gout = None
    assert r32.cap == r64.cap
    for what in ("out", "pred", "inside", "gx_num"):
        assert np.array_equal(getattr(r32, what), getattr(r64, what)), what
    for m in range(case.M):
        assert np.array_equal(r32.gw_num[m], r64.gw_num[m]), "grad_wq[%d]" % m
    if case.reach != ("above",) and case.shape != (1, 1, 1, 1):      # the case has a gradient at all (a single site may be clamped)
        assert any(np.any(g) for g in r64.gw_num) and (np.any(r64.gx_num) or case.tables_kind != "rand")


def test_cases_cross_what_they_must():
    """every interval x every u x final / non-final carries the shipped M = 3 list; the contents, shapes and clamp ends are there"""
    names = [c.name for c in fx.CASES]
    for iv in (4, 5, 6):
        mine = [c for c in fx.CASES if c.interval == iv]
        for u in (1, 2, 3, 4):
            for last in (0, 1):
                assert any(c.u == u and c.last == last and c.M == 3 for c in mine), (iv, u, last)
        assert {c.content for c in mine} >= {"noise", "natural", "extreme", "flat", "checker", "split"}
        assert {c.modes for c in mine} >= {"s", "sd", "sdy", "yds", "sdysdysd"}
        shapes = {c.shape for c in mine}
        assert (1, 1, 1, 1) in shapes and (16, 1, 48, 48) in shapes and (256, 1, 48, 48) in shapes
        assert any(s[2] == 1 and s[3] > 1 for s in shapes) and any(s[3] == 1 and s[2] > 1 for s in shapes)
        assert {s[1] for s in shapes} >= {1, 2, 3} and {s[3] for s in shapes} >= {260, 300}
        for key in ("at_lo", "at_hi", "above", "below", "band_in", "evict", "rim_lo", "rim_hi"):
            assert any(key in c.reach for c in mine), (iv, key)
        assert any("band_out" in c.reach for c in mine) == (iv != 6)      # interval 6 keeps whole tables in LDS: nothing is outside
    assert len(set(names)) == len(names)


def _host_ptrs(n):
    bufs = [ctypes.create_string_buffer(16) for _ in range(n)]       # never dereferenced: the refusals come before the device is touched
    return (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs]), bufs


@pytest.mark.parametrize("fn", ["mulut_ft_quantize", "mulut_ft_quantize_backward"])
def test_quantiser_refusals(fn):
    from mulut_amd import _native
    call = getattr(_native.load(), fn)
    EINVAL, EUNSUPPORTED = -1, -5
    w, keep_w = _host_ptrs(9)
    o, keep_o = _host_ptrs(9)
    assert call(0, w, o, 0, 4, None) == EUNSUPPORTED
    assert call(0, w, o, 9, 4, None) == EUNSUPPORTED
    assert call(0, w, o, 3, 0, None) == EINVAL
    assert call(0, w, o, 3, -1, None) == EINVAL
    assert call(0, None, o, 3, 4, None) == EINVAL
    assert call(0, w, None, 3, 4, None) == EINVAL
    for which in (0, 1):
        w2, keep_w2 = _host_ptrs(3)
        o2, keep_o2 = _host_ptrs(3)
        (w2, o2)[which][2] = None                                     # a NULL element
        assert call(0, w2, o2, 3, 4, None) == EINVAL
