"""Fine-tuning the 4 x 4 patterns e, h, o, on the CPU:
  * mulut_ft_wide_stage_forward / _backward exist, are declared and refuse what they must before any device is touched;
  * the oracle extended at run time with the taps of e, h, o (tests/ft_wide_cases.wide_oracle) computes, for all six patterns, the
    forward built from reach_cases.pass_q_np -- the NumPy restatement of a pass that tests/test_reach_cpu.py holds to c_oracle.pass_q;
  * the premise of the exact GPU tests (tests/test_gpu_ft_wide.py): on every wide case the float32 oracle equals the float64 oracle
    and the exactness cap holds;
  * mulut_amd.finetune.MuLUTWide loads, names, exports and refuses like the reference's module; MuLUT and MuLUTInterval keep their
    refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ft_wide_cases as fw
import reach_cases as rc
from oracle import ft_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EMODE, EUNSUPPORTED, ENODEVICE = -1, -2, -5, -7
NAMES = ("mulut_ft_wide_stage_forward", "mulut_ft_wide_stage_backward")


# ------------------------------------------------------------------------------------------------------------------ refusals
def _call(lib, which, interval=5, modes=b"eho", u=4, x=1, mask=1, gout=1, out=1, gx=1, gw=1, B=1, H=4, W=4):
    """The entry points with dummy non-null addresses: every refusal tested here is decided before a pointer is followed."""
    M = len(modes)
    tabs = [np.zeros(16, np.float32) for _ in range(max(M, 1))]
    ptrs = (ctypes.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
    buf = np.zeros(4096, np.float32)
    p = lambda on: ctypes.c_void_p(buf.ctypes.data if on else None)      # noqa: E731
    if which == "fwd":
        return lib.mulut_ft_wide_stage_forward(0, interval, ptrs, modes, 1, u, p(x), B, 1, H, W, p(out), p(mask), None)
    return lib.mulut_ft_wide_stage_backward(0, interval, ptrs, modes, 1, u, p(x), p(gout), p(mask), B, 1, H, W, ptrs if gw else None, p(gx), None)


def test_entry_points_are_declared_and_exported():
    from mulut_amd import _native
    lib = _native.load()
    header = open(os.path.join(ROOT, "include", "mulut.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTS and hasattr(lib, name)
        assert re.search(r"\bint %s\(int device, int interval, const float \*const \*weights_q, const char \*modes" % name, header), name
    assert "sr/model.py:119-121" in header and "sr/model.py:69-312" in header      # the citation of the reference lines they stand for


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_entry_points_refuse_before_touching_a_device(which):
    from mulut_amd import _native
    lib = _native.load()
    for interval in (3, 7):
        assert _call(lib, which, interval=interval) == EUNSUPPORTED
    for u in (0, 5):
        assert _call(lib, which, u=u) == EUNSUPPORTED
    assert _call(lib, which, modes=b"sdyehosdy") == EUNSUPPORTED      # nine: more than MULUT_MAX_MODES
    assert _call(lib, which, modes=b"") == EUNSUPPORTED
    for interval in (4, 5, 6):
        for m in (b"x", b"sxe"):
            assert _call(lib, which, interval=interval, modes=m) == EMODE
        assert _call(lib, which, interval=interval, x=0) == EINVAL
        assert _call(lib, which, interval=interval, mask=0) == EINVAL      # there is no recomputing form
        assert _call(lib, which, interval=interval, B=0) == EINVAL
        assert _call(lib, which, interval=interval, H=0) == EINVAL
        assert _call(lib, which, interval=interval, W=-3) == EINVAL
        if which == "bwd":
            assert _call(lib, which, interval=interval, gout=0) == EINVAL
            assert _call(lib, which, interval=interval, gx=0) == EINVAL
            assert _call(lib, which, interval=interval, gw=0) == EINVAL
        else:
            assert _call(lib, which, interval=interval, out=0) == EINVAL
    # the order of the checks is that of the other stage entry points: a NULL pointer before the interval, the interval before the mode
    assert _call(lib, which, interval=7, x=0) == EINVAL
    assert _call(lib, which, interval=7, modes=b"x") == EUNSUPPORTED
    if not torch.cuda.is_available():
        for interval in (4, 5, 6):
            for m in (b"eho", b"sdy", b"sdyehoeh"):
                assert _call(lib, which, interval=interval, modes=m) == ENODEVICE      # well-formed: only the device is missing (no CPU path)


def test_the_narrow_entry_points_still_refuse_wide_modes():
    """e, h, o at the six existing stage entry points stay MULUT_EMODE (tests/test_ft_interval_cpu.py pins the interval pair)."""
    from mulut_amd import _native
    lib = _native.load()
    buf = np.zeros(4096, np.float32)
    b = ctypes.c_void_p(buf.ctypes.data)
    ptrs = (ctypes.c_void_p * 3)(*[buf.ctypes.data] * 3)
    for m in (b"e", b"h", b"o", b"sde"):
        assert lib.mulut_ft_stage_forward(0, ptrs, m, 1, 4, b, 1, 1, 4, 4, b, None) == EMODE
        assert lib.mulut_ft_stage_forward_mask(0, ptrs, m, 1, 4, b, 1, 1, 4, 4, b, b, None) == EMODE
        assert lib.mulut_ft_stage_backward(0, ptrs, m, 1, 4, b, b, 1, 1, 4, 4, ptrs, b, None) == EMODE
        assert lib.mulut_ft_stage_backward_mask(0, ptrs, m, 1, 4, b, b, b, 1, 1, 4, 4, ptrs, b, None) == EMODE


# ---------------------------------------------------------------------------------------------------------- the oracle extension
def test_wide_oracle_restores_the_pinned_oracle():
    before = (dict(ft_torch.PATTERNS), dict(ft_torch.PAD))
    with fw.wide_oracle() as o:
        assert o is ft_torch and sorted(ft_torch.PATTERNS) == sorted("sdyeho") and ft_torch.PAD["e"] == 3
        assert {m: ft_torch.PATTERNS[m] for m in "eho"} == {m: rc.PATTERNS[m] for m in "eho"}      # the taps the inference tests use
        assert {m: ft_torch.PATTERNS[m] for m in "sdy"} == before[0]
    assert (ft_torch.PATTERNS, ft_torch.PAD) == before and sorted(ft_torch.PATTERNS) == sorted("sdy")
    with pytest.raises(ValueError, match="Mode e not implemented"):
        ft_torch.interp_batch(torch.zeros(17 ** 4, 1), 1, "e", torch.zeros(1, 1, 4, 4), 3)


@pytest.mark.parametrize("interval", fw.INTERVALS)
@pytest.mark.parametrize("u", [1, 2, 3, 4])
def test_extended_oracle_equals_the_numpy_pass_forward(interval, u):
    """The un-clamped pred of ft_torch.stage(quantised=True) under wide_oracle() against p = round(p + pass_q / q) per pass in
    float32, pass_q from reach_cases.pass_q_np, on all six patterns in one list and on each wide pattern alone."""
    q, L = 2 ** interval, 2 ** (8 - interval) + 1
    rng = np.random.default_rng(100 * interval + u)
    img = rng.integers(0, 256, (2, 7, 9), dtype=np.uint8)      # [C][H][W]
    img[0, :2, :3] = (0, 255, q)                                # both ends of the grid
    for modes in ("sdyeho", "e", "h", "o"):
        tabs = [rng.integers(-127, 128, (L ** 4, u * u), dtype=np.int8) for _ in modes]
        p = np.zeros((2, 7 * u, 9 * u), np.float32)
        for t, m in zip(tabs, modes):
            for r in range(4):
                p = np.round(p + rc.pass_q_np(t, img, r, u, m, interval).astype(np.float32) / np.float32(q)).astype(np.float32)
        with fw.wide_oracle():
            _, pred = ft_torch.stage([torch.from_numpy(t.astype(np.float32)) for t in tabs], torch.from_numpy(img[None].astype(np.float32)),
                                     modes, True, u, interval, quantised=True)
        # (== on float32: every value, the sign of a zero apart -- round(-0.3) is -0.0 in NumPy and 0.0 after the oracle's x + (round(x) - x))
        assert pred.dtype == torch.float32 and np.array_equal(pred.numpy()[0], p), (modes, int((pred.numpy()[0] != p).sum()))


# ----------------------------------------------------------------------------------------------------------- exactness premise
@pytest.mark.parametrize("case", fw.CASES, ids=lambda c: c.name)
def test_float32_oracle_equals_float64_oracle_exactly(case):
    case.build()
    try:
        r64 = fw.reference(case, dtype=torch.float64)      # asserts integrality, the cap and the case's reach
        r32 = fw.reference(case, dtype=torch.float32, check_reach=False)
    finally:
        case.tables = case.x = case.gout = None
    assert r64.cap < fw.CAP and r32.cap == r64.cap
    assert r64.cap > 0 or case.reach == ("above",)      # (every element clamped: no gradient, by construction)
    for what in ("out", "pred", "inside", "gx_num"):
        assert np.array_equal(getattr(r32, what), getattr(r64, what)), what
    for m in range(case.M):
        assert np.array_equal(r32.gw_num[m], r64.gw_num[m]), "grad_wq[%d]" % m
    if case.shape == (1, 1, 1, 1):
        assert r64.inside.any()      # the one site's mask is not empty: the case has gradients
    if case.reach != ("above",):
        assert any(np.any(g) for g in r64.gw_num) and (np.any(r64.gx_num) or case.tables_kind != "rand")


def test_cases_cross_what_they_must():
    names = [c.name for c in fw.CASES]
    assert len(set(names)) == len(names)
    for iv in fw.INTERVALS:
        mine = [c for c in fw.CASES if c.interval == iv]
        assert all(set(c.modes) & set("eho") for c in mine)      # every case needs the halo of 3
        shapes = {c.shape for c in mine}
        assert {(1, 1, 1, 1), (1, 3, 2, 2), (1, 2, 9, 11), (2, 1, 13, 10), (1, 1, 5, 6), (2, 1, 5, 6), (1, 2, 3, 300), (1, 1, 4, 260),
                (1, 1, 2, 120), (16, 1, 48, 48), (64, 1, 48, 48)} <= shapes
        assert {c.u for c in mine} == {1, 2, 3, 4} and {c.modes for c in mine} >= {"e", "ho", "sdyeho", "eho", "oeh", "sdyehoeh"}
        for key in ("at_lo", "at_hi", "above", "below", "band_in", "evict", "rim_lo", "rim_hi"):
            assert any(key in c.reach for c in mine), (iv, key)
        assert any("band_out" in c.reach for c in mine) == (iv != 6)
        # the wave tile: (rows + 6) * (W + 6) floats against 1024 -- one case that still fits at halo 3 and not at 4, the wide ones that do not
        assert (2 + 6) * (120 + 6) <= 1024 < (2 + 8) * (120 + 8) and (1 + 6) * (260 + 6) > 1024


# --------------------------------------------------------------------------------------------------------------------- classes
def _lut(interval, stage, mode, vnum):
    rng = np.random.default_rng(1000 * interval + 17 * stage + ord(mode))
    return rng.integers(-128, 128, size=((2 ** (8 - interval) + 1) ** 4, vnum), dtype=np.int8)


def test_module_class_loads_names_exports_and_refuses(tmp_path):
    import mulut_amd
    from mulut_amd import finetune
    assert mulut_amd.MuLUTWide is finetune.MuLUTWide and issubclass(finetune.MuLUTWide, torch.nn.Module)
    for interval in (5, 6):
        for s in (1, 2):
            for m in "seho":
                np.save(tmp_path / ("LUT_x2_%dbit_int8_s%d_%s.npy" % (interval, s, m)), _lut(interval, s, m, 4 if s == 2 else 1))
    for interval, rows in ((5, 6561), (6, 625)):
        net = finetune.MuLUTWide(str(tmp_path), 2, "seho", upscale=2, interval=interval)
        assert sorted(n for n, _ in net.named_parameters()) == sorted("weight_s%d_%s" % (s, m) for s in (1, 2) for m in "seho")
        assert net.weight_s2_h.shape == (rows, 4) and net.weight_s1_o.shape == (rows, 1) and net.weight_s2_e.dtype == torch.float32
        assert np.array_equal(net.weight_s2_e.detach().numpy(), _lut(interval, 2, "e", 4).astype(np.float32) / np.float32(127.0))
        exp = net.export_int8()
        assert sorted(exp) == sorted("s%d_%s" % (s, m) for s in (1, 2) for m in "seho")
        assert exp["s2_o"].dtype == np.int8 and np.array_equal(exp["s2_o"], np.maximum(_lut(interval, 2, "o", 4), -127))
        with pytest.raises(RuntimeError, match="no CPU path"):
            net(torch.zeros(1, 1, 4, 4))
    assert finetune.MuLUTWide(str(tmp_path), 2, list("eh"), upscale=2, interval=6).modes == "eh"      # a list of letters, as the reference passes it
    with pytest.raises(ValueError, match=r"Mode x not implemented\."):
        finetune.MuLUTWide(str(tmp_path), 2, "ex", upscale=2, interval=5)
    for interval in (3, 7):
        with pytest.raises(ValueError, match="interval 4, 5 or 6"):
            finetune.MuLUTWide(str(tmp_path), 2, "eho", upscale=2, interval=interval)
    # the s, d, y classes keep their refusals
    with pytest.raises(ValueError, match="Mode e not implemented"):
        finetune.MuLUT(str(tmp_path), 2, "se", upscale=2, interval=4)
    for interval in (5, 6):
        with pytest.raises(ValueError, match="Mode e not implemented"):
            finetune.MuLUTInterval(str(tmp_path), 2, "se", upscale=2, interval=interval)


def test_driver_picks_the_wide_class_only_for_wide_lists(tmp_path, monkeypatch):
    from mulut_amd import finetune_lut
    picked = []

    class Stop(Exception):
        pass

    def record(cls):
        def make(*a, **k):
            picked.append((cls, k.get("interval")))
            raise Stop()
        return make

    for cls in ("MuLUT", "MuLUTInterval", "MuLUTWide"):
        monkeypatch.setattr(finetune_lut, cls, record(cls))
    for modes, interval in (("sdy", 4), ("sdy", 5), ("s", 6), ("eho", 4), ("sdyeho", 5), ("sh", 6)):
        with pytest.raises(Stop):
            finetune_lut.main(["--modes", modes, "--interval", str(interval), "-e", str(tmp_path), "--trainDir", str(tmp_path)])
    assert picked == [("MuLUT", 4), ("MuLUTInterval", 5), ("MuLUTInterval", 6), ("MuLUTWide", 4), ("MuLUTWide", 5), ("MuLUTWide", 6)]
