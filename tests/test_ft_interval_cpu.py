"""Fine-tuning at the sampling intervals 5 and 6 on the CPU:
  * oracle/ft_torch.py at interval 5 / 6 against outputs AND gradients of the reference's own module
    (tests/golden/ft_interval_fixtures.npz, produced by tests/golden/gen_golden_ft_interval.py) at the bars of test_oracle_ft.py;
  * the per-pass set-up the kernels are built from (mulut_ft_interval.h, compiled by g++ as tests/host_emul/emul_ft_interval.cpp)
    against the oracle's rank table and interpolation, for every tie pattern;
  * the two C entry points and the Python class refuse what they must, before any device is touched."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from host_emul_lib import load_emul_ft_interval
from oracle import ft_torch

CASES = ["A5_s2sdy_x4_u8", "A6_s2sdy_x4_u8", "C5_s2sd_x2_u8", "B6_s1s_x3_float", "E5_s3y_x1_grid"]


def synthetic_lut(interval, stage, mode, vnum):
    rng = np.random.default_rng(1000 * interval + 17 * stage + ord(mode))
    return rng.integers(-128, 128, size=((2 ** (8 - interval) + 1) ** 4, vnum), dtype=np.int8)


def tables_for(fx, name):
    interval, stages, scale = [int(v) for v in fx[name + "/cfg"]]
    modes = bytes(fx[name + "/modes"]).decode()
    src = bytes(fx[name + "/lutsrc"]).decode()
    iv_fx = np.load(os.path.join(GOLDEN, "interval_fixtures.npz")) if src == "transferred" else None
    out = {}
    for s in range(stages):
        vnum = scale * scale if s + 1 == stages else 1
        for m in modes:
            key = "s%d_%s" % (s + 1, m)
            t = iv_fx["iv%d/lut/%s" % (interval, key)] if iv_fx is not None else synthetic_lut(interval, s + 1, m, vnum)
            out[key] = np.ascontiguousarray(t.reshape(-1, vnum).astype(np.int8))
    return out, interval, stages, modes, scale


def test_fixture_file_holds_the_cases_of_both_intervals():
    fx = np.load(os.path.join(GOLDEN, "ft_interval_fixtures.npz"))
    assert sorted({k.split("/")[0] for k in fx.files}) == sorted(CASES)
    assert {int(fx[n + "/cfg"][0]) for n in CASES} == {5, 6}
    assert os.path.getsize(os.path.join(GOLDEN, "ft_interval_fixtures.npz")) < 1000000
    x = fx["E5_s3y_x1_grid/x"] * np.float32(255)
    assert set(np.unique(np.round(x)).astype(int)) <= {0, 31, 32, 224, 255}
    assert any((synthetic_lut(5, s, m, 1) == -128).any() for s in (1, 2) for m in "sd")      # the quantiser's clamp is exercised


@pytest.mark.parametrize("name", CASES)
def test_ft_oracle_matches_reference_at_intervals_5_and_6(name):
    fx = np.load(os.path.join(GOLDEN, "ft_interval_fixtures.npz"))
    tabs, interval, stages, modes, scale = tables_for(fx, name)
    rows = (2 ** (8 - interval) + 1) ** 4
    weights = {k: torch.from_numpy(v.astype(np.float32) / 127.0).requires_grad_(True) for k, v in tabs.items()}
    x = torch.from_numpy(fx[name + "/x"]).requires_grad_(True)
    y = ft_torch.forward(weights, x, stages, modes, scale, interval)
    assert np.array_equal(y.detach().numpy(), fx[name + "/y"])
    loss = torch.nn.functional.mse_loss(y, torch.from_numpy(fx[name + "/target"]))
    loss.backward()
    assert abs(loss.item() - float(fx[name + "/loss"])) < 1e-7
    assert np.allclose(x.grad.numpy(), fx[name + "/grad_x"], rtol=1e-5, atol=1e-9)
    for key, w in weights.items():
        assert w.shape[0] == rows
        dense = np.zeros((rows, w.shape[1]), np.float32)
        dense[fx[name + "/grad/" + key + "/rows"]] = fx[name + "/grad/" + key + "/vals"]
        assert np.allclose(w.grad.numpy(), dense, rtol=1e-5, atol=1e-9), key


@pytest.fixture(scope="module")
def emul_ft_iv():
    L = load_emul_ft_interval()
    L.emul_ft_interval_passes.restype = ctypes.c_int
    L.emul_ft_interval_passes.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long] + [ctypes.c_void_p] * 4
    return L


def run_passes(L, interval, v):
    v = np.ascontiguousarray(v, np.float32)
    n = len(v)
    idx, wt = np.empty((n, 5), np.int32), np.empty((n, 5), np.float32)
    order, corner = np.empty((n, 4), np.int32), np.empty((n, 5), np.int32)
    assert L.emul_ft_interval_passes(interval, v.ctypes.data, n, idx.ctypes.data, wt.ctypes.data, order.ctypes.data, corner.ctypes.data) == 0
    return idx, wt, order, corner


def oracle_passes(interval, v):
    """rows, weights and rank order as oracle/ft_torch.py computes them (interp_batch's own expressions, :48-61)."""
    q, L = 2 ** interval, 2 ** (8 - interval) + 1
    t = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    msb = torch.floor_divide(t, q).long()
    lsb = t % q
    order = ft_torch._case_order(lsb[..., 0], lsb[..., 1], lsb[..., 2], lsb[..., 3])
    strides = torch.tensor([L ** 3, L ** 2, L, 1], dtype=torch.long)
    fs = torch.gather(lsb, -1, order)
    base = (msb * strides).sum(-1)
    idx = torch.cat([base[..., None], base[..., None] + torch.cumsum(strides[order], -1)], -1)
    wt = torch.cat([q - fs[..., :1], fs[..., :-1] - fs[..., 1:], fs[..., 3:]], -1)
    return idx.numpy(), wt.numpy(), order.numpy(), msb.numpy()


@pytest.mark.parametrize("interval", [5, 6])
def test_pass_setup_equals_the_oracle_for_every_tie_pattern(emul_ft_iv, interval):
    """Every 4-tuple of fractional parts over a set with ties, each with several random MSB quadruples (both ends of the grid
    included), plus non-integer values: the five rows, the five weights (bit for bit) and the rank order are the oracle's."""
    q, L = 2 ** interval, 2 ** (8 - interval) + 1
    rng = np.random.default_rng(interval)
    fr = np.array(list(itertools.product([0, 1, q // 2, q - 1], repeat=4)), np.float32)      # 256 tie patterns
    vs = []
    for h in ([0, 0, 0, 0], [L - 2] * 4, None, None, None, None):
        msb = np.array(h, np.float32) if h is not None else rng.integers(0, L - 1, (len(fr), 4)).astype(np.float32)
        vs.append(msb * q + fr)
    vs.append(rng.random((4096, 4), dtype=np.float32) * np.float32(255))                       # inputs need not be integers
    half = rng.integers(0, 511, (2048, 4)).astype(np.float32) / np.float32(2)                   # halves: exact ties off the integers
    vs.append(half)
    v = np.concatenate(vs)
    assert v.min() >= 0 and v.max() <= 255
    idx, wt, order, corner = run_passes(emul_ft_iv, interval, v)
    want_idx, want_wt, want_order, msb = oracle_passes(interval, v)
    assert np.array_equal(order, want_order)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(wt.view(np.int32), want_wt.view(np.int32))
    assert idx.min() >= 0 and idx.max() < L ** 4
    # the corner code of a vertex is the parity of its MSB coordinates: five different codes per pass, and row -> code is a function
    coords = np.stack([idx // L ** 3, idx // L ** 2 % L, idx // L % L, idx % L], -1)
    assert np.array_equal(corner, ((coords & 1) * np.array([8, 4, 2, 1])).sum(-1))
    assert all(len(set(c)) == 5 for c in corner)


def test_pass_setup_weights_interpolate_like_the_oracle(emul_ft_iv):
    """sum_j wt_j * table[idx_j] / q in the reference's association equals interp_batch on a 1 x 1 crop, bit for bit."""
    for interval in (5, 6):
        q, L = 2 ** interval, 2 ** (8 - interval) + 1
        rng = np.random.default_rng(10 + interval)
        tab = rng.integers(-127, 128, (L ** 4, 1)).astype(np.float32)
        v = rng.integers(0, 256, (500, 4)).astype(np.float32)
        idx, wt, _, _ = run_passes(emul_ft_iv, interval, v)
        rows = tab[idx, 0]
        got = ((((wt[:, 0] * rows[:, 0] + wt[:, 1] * rows[:, 1]) + wt[:, 2] * rows[:, 2]) + wt[:, 3] * rows[:, 3]) + wt[:, 4] * rows[:, 4]) / np.float32(q)
        img = torch.from_numpy(v.reshape(500, 1, 2, 2))      # keys a, b, c, d of pattern s are the 2 x 2 crop
        want = ft_torch.interp_batch(torch.from_numpy(tab / np.float32(127.0)), 1, "s", img, 1, interval).reshape(-1).numpy()
        assert np.array_equal(got.astype(np.float32), want)


def _call(lib, which, interval=5, modes=b"sdy", u=4, x=1, mask=1, gout=1, B=1, H=4, W=4):
    """The entry points with dummy non-null addresses: every refusal tested here is decided before a pointer is followed."""
    M = len(modes)
    rows = (2 ** (8 - interval) + 1) ** 4 if interval in (5, 6) else 1
    tabs = [np.zeros((rows, u * u if 1 <= u <= 4 else 1), np.float32) for _ in range(max(M, 1))]
    ptrs = (ctypes.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
    buf = np.zeros(4096, np.float32)
    p = lambda on: ctypes.c_void_p(buf.ctypes.data if on else None)      # noqa: E731
    if which == "fwd":
        return lib.mulut_ft_interval_stage_forward(0, interval, ptrs, modes, 1, u, p(x), B, 1, H, W, p(1), p(mask), None)
    return lib.mulut_ft_interval_stage_backward(0, interval, ptrs, modes, 1, u, p(x), p(gout), p(mask), B, 1, H, W, ptrs, p(1), None)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_entry_points_refuse_before_touching_a_device(which):
    from mulut_amd import _native
    lib = _native.load()
    assert "mulut_ft_interval_stage_forward" in _native.EXPORTS and "mulut_ft_interval_stage_backward" in _native.EXPORTS
    EINVAL, EMODE, EUNSUPPORTED, ENODEVICE = -1, -2, -5, -7
    assert _call(lib, which, interval=4) == EUNSUPPORTED          # interval 4 stays with mulut_ft_stage_*
    assert _call(lib, which, interval=7) == EUNSUPPORTED
    for m in (b"e", b"h", b"o", b"sxe"):
        assert _call(lib, which, modes=m) == EMODE
    assert _call(lib, which, u=5) == EUNSUPPORTED
    assert _call(lib, which, u=0) == EUNSUPPORTED
    assert _call(lib, which, modes=b"sdysdysdy") == EUNSUPPORTED   # more than MULUT_MAX_MODES
    assert _call(lib, which, x=0) == EINVAL
    assert _call(lib, which, mask=0) == EINVAL
    assert _call(lib, which, B=0) == EINVAL
    assert _call(lib, which, W=-3) == EINVAL
    if which == "bwd":
        assert _call(lib, which, gout=0) == EINVAL
    if not torch.cuda.is_available():
        for interval in (5, 6):
            assert _call(lib, which, interval=interval) == ENODEVICE      # well-formed: only the device is missing (no CPU path)


def test_module_classes_refuse(tmp_path):
    from mulut_amd import MuLUTInterval
    from mulut_amd import finetune
    assert MuLUTInterval is finetune.MuLUTInterval
    for interval in (4, 7):
        with pytest.raises(ValueError, match="interval 5 or 6"):
            finetune.MuLUTInterval(str(tmp_path), 2, "sdy", upscale=4, interval=interval)
    for interval in (5, 6):
        with pytest.raises(ValueError, match="Mode e not implemented"):
            finetune.MuLUTInterval(str(tmp_path), 2, "se", upscale=4, interval=interval)
        with pytest.raises(NotImplementedError, match="interval-4 only"):
            finetune.MuLUT(str(tmp_path), 2, "sdy", upscale=4, interval=interval)
    # tables load under the writer-side name, [L^4, u*u] float32 = int8 / 127, and export_int8 gives them back
    for m in "sd":
        np.save(tmp_path / ("LUT_x2_6bit_int8_s1_%s.npy" % m), synthetic_lut(6, 1, m, 4))
    net = finetune.MuLUTInterval(str(tmp_path), 1, "sd", upscale=2, interval=6)
    assert sorted(n for n, _ in net.named_parameters()) == ["weight_s1_d", "weight_s1_s"]
    assert net.weight_s1_s.shape == (625, 4) and net.weight_s1_s.dtype == torch.float32
    assert np.array_equal(net.export_int8()["s1_d"], np.maximum(synthetic_lut(6, 1, "d", 4), -127))
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.zeros(1, 1, 4, 4))
