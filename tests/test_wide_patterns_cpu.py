"""The 4 x 4 sampling patterns e, h, o (reach 3) on the CPU: the per-site math of mulut_core.h (tests/host_emul) against the
NumPy port of the reference's inference loop, the LUT producer against tables the reference's own network code produced
(tests/golden/wide_fixtures.npz, gen_golden_wide.py), and the inference offsets against that network's output on grid-aligned
images.  oracle/np_port.py takes its pattern table from module-level dicts; e, h, o are added to them here for the test only."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import np_port
from test_core_math_cpu import emul, run_emul  # noqa: F401  (the host emulator fixture and driver)

from mulut_amd import network, transfer_to_lut as T

WIDE_PATTERNS = {"e": ((0, 0), (0, 3), (3, 0), (3, 3)), "h": ((0, 0), (2, 2), (2, 3), (3, 2)), "o": ((0, 0), (2, 2), (1, 3), (3, 1))}


@pytest.fixture
def np_wide(monkeypatch):
    for m, taps in WIDE_PATTERNS.items():
        monkeypatch.setitem(np_port.PATTERNS, m, taps)
        monkeypatch.setitem(np_port.PAD, m, 3)
    return np_port


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "wide_fixtures.npz"))


def _tables(seed, modes, u):
    rng = np.random.default_rng(seed)
    return {m: rng.integers(-127, 128, (17 ** 4, u * u)).astype(np.int8) for m in set(modes)}


def _np_stage(np_mod, tabs, modes, is_last, img, u):
    """One stage of np_port.run_stages (the reference's loop) with the given tables."""
    lut = {"s1_" + m: t.astype(np.float32) for m, t in tabs.items()}
    if is_last:
        return np_mod.run_stages(lut, 1, modes, u, img)
    # a non-final stage is stage 1 of a 2-stage cascade: its own output is the first of return_all
    lut.update({"s2_" + m: np.zeros((17 ** 4, 1), np.float32) for m in tabs})
    return np_mod.run_stages(lut, 2, modes, 1, img, return_all=True)[0]


@pytest.mark.parametrize("modes", ["e", "h", "o", "eho", "sdyeho", "sdyehoeh"])
@pytest.mark.parametrize("u,is_last", [(1, False), (1, True), (2, True), (3, True), (4, True)])
def test_emulator_matches_np_port(emul, np_wide, modes, u, is_last):  # noqa: F811
    rng = np.random.default_rng(len(modes) * 10 + u)
    img = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    img[:4, :5] = img[0, 0]                                     # a flat patch: passes at grid vertices as well
    tabs = _tables(u + 7 * len(modes), modes, u)
    got = run_emul(emul, [tabs[m] for m in modes], modes, is_last, img, u)
    want = _np_stage(np_wide, tabs, modes, is_last, img, u)
    assert np.array_equal(got, want), (modes, u, is_last)


@pytest.mark.parametrize("shape", [(1, 1, 1), (4, 3, 2), (7, 5, 1)])
def test_emulator_odd_sizes(emul, np_wide, shape):  # noqa: F811
    img = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    for modes, u, last in (("eho", 1, False), ("sdyeho", 3, True), ("oe", 4, True)):
        tabs = _tables(u, modes, u)
        assert np.array_equal(run_emul(emul, [tabs[m] for m in modes], modes, last, img, u),
                              _np_stage(np_wide, tabs, modes, last, img, u)), (shape, modes, u)


def _opt(stages, modes, scale):
    return SimpleNamespace(stages=stages, modes=modes, scale=scale, interval=4, expDir="")


def test_mode_input_tensor_taps():
    x = T.get_input_tensor(_opt(1, "e", 2))[:300:7]
    for m, taps in WIDE_PATTERNS.items():
        p = T.get_mode_input_tensor(x, m)
        assert p.shape == (x.shape[0], 1, 4, 4)
        mask = torch.zeros(4, 4, dtype=torch.bool)
        for k, (i, j) in enumerate(taps):
            assert torch.equal(p[:, 0, i, j], x[:, 0, k // 2, k % 2]), (m, k)
            mask[i, j] = True
        assert (p[:, 0][:, ~mask] == 0).all(), m
    with pytest.raises(ValueError, match="Mode s not implemented"):
        T.get_mode_input_tensor(x, "s")


def _tiny_twin(fx):
    net = network.SRNets(nf=8, scale=2, modes=list("eho"), stages=2)
    sd = {k[len("tinyw/"):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("tinyw/")}
    net.load_state_dict(sd, strict=True)
    return net


@pytest.fixture(scope="module")
def tiny_tables(fx):
    return T.transfer(_tiny_twin(fx), _opt(2, "eho", 2), save=False)


def test_tiny_model_tables_match_reference(fx, tiny_tables):
    """The same bar as tests/test_transfer_cpu.py: a table entry is round(127 tanh(...)), and a different summation order in
    the matrix products may move a value within float rounding of a .5 boundary by one step: no entry off by more than 1,
    at most 0.01 % of the entries off at all."""
    for key, t in tiny_tables.items():
        ref = "tiny/" + key
        assert tuple(t.shape) == tuple(fx[ref + "/shape"]) and t.dtype == np.int8, key
        rows = t.reshape(t.shape[0], -1)[fx["idx"]].astype(np.int32)
        diff = np.abs(rows - fx[ref + "/rows"].astype(np.int32))
        assert diff.max() <= 1 and (diff != 0).mean() <= 1e-4, (key, diff.max(), (diff != 0).mean())
    assert sorted(tiny_tables) == ["s1_e", "s1_h", "s1_o", "s2_e", "s2_h", "s2_o"]


def test_transfer_writes_wide_tables(fx, tmp_path):
    opt = SimpleNamespace(stages=2, modes="sdyeho", scale=2, interval=4, expDir=str(tmp_path))
    net = network.SRNets(nf=4, scale=2, modes=list("sdyeho"), stages=2)
    T.transfer(net, opt)
    names = sorted(os.listdir(str(tmp_path)))
    assert names == sorted("LUT_x2_4bit_int8_s%d_%s.npy" % (s, m) for s in (1, 2) for m in "sdyeho")
    assert np.load(os.path.join(str(tmp_path), "LUT_x2_4bit_int8_s2_h.npy")).shape == (17 ** 4, 1, 2, 2)


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("mode", ["e", "h", "o"])
def test_grid_image_inference_equals_reference_network(fx, np_wide, tiny_tables, stage, mode):
    """On a grid-aligned image every pass puts weight 16 on one table vertex, so the rotation-0 pass of the transferred table
    equals 16 x the reference network's own output at every interior site -- up to the 1-LSB (x 16) allowance for a table entry
    that the GEMM form rounds differently from the reference's convolution (see test_tiny_model_tables_match_reference)."""
    img = fx["img/s%d_%s" % (stage, mode)].astype(np.float32)
    net_out = fx["netout/s%d_%s" % (stage, mode)].astype(np.int64)
    u = 1 if stage == 1 else 2
    H, W = img.shape
    table = tiny_tables["s%d_%s" % (stage, mode)].reshape(17 ** 4, u * u).astype(np.float32)
    padded = np.pad(img, ((0, 3), (0, 3)), mode="edge")[None]
    q = np_wide.four_simplex_interp(table, padded, H, W, 4, 4, upscale=u, mode=mode) * 16     # q * pass, rotation 0
    got = np.rint(q[0, :(H - 3) * u, :(W - 3) * u]).astype(np.int64)
    assert net_out.shape == got.shape
    diff = np.abs(got - 16 * net_out)
    assert diff.max() <= 16 and (diff != 0).mean() <= 0.01, (diff.max(), (diff != 0).mean())


def test_finetune_module_refuses_wide_modes(tmp_path):
    """Fine-tuning stays with s, d, y: the module raises as the reference's does for a mode it lacks (sr/model.py:121)."""
    from mulut_amd.finetune import MuLUT
    for modes in ("e", "sdh", "sdyo"):
        with pytest.raises(ValueError, match="Mode [eho] not implemented"):
            MuLUT(str(tmp_path), 2, modes, upscale=4)
