"""The cases and the comparison of tests/net_grid_cases.py without a GPU: the models of tests/ reach every compiled (MT, U) instance,
the float32 torch path stays within MEASURED_Y of float64 and itself passes the decided-exact comparison, no case leaves more than
1 % of its values undecided, the op-level cases of the new models stay inside the gradient bars of net_train_cases.py, and the
comparison catches four mutations of the float64 restatement -- the first of which the statistical bar of net_cases.meets lets pass."""
import numpy as np
import pytest
import torch

from mulut_amd import network
import net_cases as nc
import net_grid_cases as gc
import net_train_cases as tc


def test_the_models_of_the_suite_reach_all_eight_instances():
    """(MT, U) of every stage of nc.MODELS, SEEDED, OP_MODELS and GRID_MODELS.  The last stages give seven pairs; (1, 1) can only be a
    stage before the last (u = 1 there), which the two-stage nf 8 models have."""
    lists = dict(fixture=list(nc.MODELS.values()), seeded=gc.SEEDED, op=tc.OP_MODELS, grid=gc.GRID_MODELS)
    every, last = set(), set()
    for name, cfgs in lists.items():
        for cfg in cfgs:
            p = gc.pairs(cfg)
            print("%s %s: %r" % (name, tc.model_id(dict(cfg, modes=cfg["modes"])), p))
            every.update(p)
            last.add(p[-1])
    assert every == gc.ALL_PAIRS, sorted(gc.ALL_PAIRS - every)
    assert last == gc.ALL_PAIRS - {(1, 1)}, sorted(gc.ALL_PAIRS - last)
    assert [gc.pairs(c)[-1] for c in gc.GRID_MODELS] == [(1, 4), (2, 2), (2, 3), (1, 2)]
    assert {c["nf"] for c in gc.GRID_MODELS} >= {1, 32} and all(c["stages"] == 1 for c in gc.GRID_MODELS)
    assert gc.T == 8 * gc.MEASURED_Y


def test_float32_torch_path_against_float64():
    """Over every stage of GRID_MODELS and SEEDED on GRID_SHAPES: |127 y32 - 127 y64| <= MEASURED_Y (T is 8 x that), the float32 path
    passes the decided-exact comparison per model, and no model leaves more than 1 % of its values undecided (a share is taken over
    all the values a model has on GRID_SHAPES: of the 48 values of a 1 x 3 x 1 x 1 case a single one is 2 %)."""
    worst = (0.0, None)
    for cfg in gc.GRID_MODELS + gc.SEEDED:
        net = gc.nets(cfg)[0]
        got, want, undecided = [], [], 0
        for shape in gc.GRID_SHAPES:
            for s, (x, v64, _) in enumerate(gc.forward_case(cfg, shape), 1):
                v32 = gc.terms(net, x, cfg["modes"], s, torch.float32).numpy()
                d = float(np.abs(v32.astype(np.float64) - v64).max())
                worst = max(worst, (d, (tc.model_id(cfg), shape, s)))
                got.append(np.rint(v32).ravel())
                want.append(v64.ravel())
        undecided = gc.exact_where_decided(np.concatenate(got), np.concatenate(want), tc.model_id(cfg) + " float32 torch path")
        assert undecided <= gc.MAX_UNDECIDED * sum(w.size for w in want)
    print("float32 torch against float64: largest |127 y32 - 127 y64| %.3g at %r (MEASURED_Y %.3g, T %.3g)" % (worst[0], worst[1], gc.MEASURED_Y, gc.T))
    assert worst[0] <= gc.MEASURED_Y


def test_new_op_cases_stay_inside_the_gradient_bars():
    """op_case / op_reference of net_train_cases.py on GRID_MODELS x GRID_SHAPES in float32 against float64: inside MEASURED_P,
    MEASURED_X and MAX_DROP as they stand, so tc.C applies to the GPU tests of these models unchanged.  Likewise the two stages that
    only the C ABI can express."""
    worst_p, worst_x, most = 0.0, 0.0, 0.0
    for cfg in gc.GRID_MODELS:
        for shape in gc.GRID_SHAPES:
            case = tc.op_case(cfg, shape, 1)
            assert case["dropped"] <= tc.MAX_DROP, (tc.model_id(cfg), shape, case["dropped"])
            most = max(most, case["dropped"])
            gx, gp = tc.op_reference(case["net"], case["x"], case["g"], cfg["modes"], 1)
            worst_x = max(worst_x, tc.distance(gx, case["gx64"]))
            worst_p = max([worst_p] + [tc.distance(gp[n], case["gp64"][n]) for n in gp])
    print("float32 torch against float64: parameters %.3g, gx %.3g of max |ref|; at most %.3g of a case's pixels dropped" % (worst_p, worst_x, most))
    assert worst_p <= tc.MEASURED_P and worst_x <= tc.MEASURED_X
    for spec in (gc.EIGHT, gc.MIXED):
        case = gc.multi_case(spec, (2, 3, 5, 7))
        assert case["dropped"] <= tc.MAX_DROP and case["v64"].shape[0] == 4 * len(gc.multi_modes(spec)), gc.multi_id(spec)
        assert sum(len(g) for g in case["gp64"]) == 12 * len(gc.multi_modes(spec))
    assert len(gc.multi_modes(gc.EIGHT)) == 8 and {gc.pairs(c)[0] for c, _ in gc.MIXED} == {(1, 2)} and len({c["nf"] for c, _ in gc.MIXED}) == 2


# ------------------------------------------------------------------------------------------------------------------- mutations
SY = gc.GRID_MODELS[0]      # nf 32 x4 "sy"


def _fails(got, v64, what):
    with pytest.raises(AssertionError, match="decided values wrong"):
        gc.exact_where_decided(got, v64, what)


def test_one_decided_value_off_by_one_is_caught_and_passes_the_old_bar():
    (x, v64, _), = gc.forward_case(SY, (1, 1, 33, 65))
    good = gc.rounded(v64)
    gc.exact_where_decided(good, v64, "unmutated")
    i = int(np.flatnonzero(gc.decided(v64).ravel() & (np.abs(good.ravel()) < 127))[1234])
    bad = good.copy().ravel()
    bad[i] += 1
    bad = bad.reshape(good.shape)
    nc.meets(bad, good, nc.BAR, "one value off by one under the statistical bar")      # the gap: 1 of 274,560 is a share of 3.6e-6
    _fails(bad, v64, "one decided value off by one")


def test_zero_padding_is_caught(monkeypatch):
    (x, v64, _), = gc.forward_case(SY, (1, 1, 1, 9))
    pad = tc.F.pad
    monkeypatch.setattr(tc.F, "pad", lambda t, p, mode: pad(t, p, mode="constant", value=0.0))
    zero = gc.terms(gc.nets(SY)[1], x, SY["modes"], 1, torch.float64).numpy()
    monkeypatch.undo()
    assert np.array_equal(gc.terms(gc.nets(SY)[1], x, SY["modes"], 1, torch.float64).numpy(), v64)
    _fails(gc.rounded(zero), v64, "zero padding")


def test_a_block_of_rotation_1_not_rotated_back_is_caught():
    (x, v64, _), = gc.forward_case(SY, (2, 3, 5, 7))
    N, C, H, W = x.shape
    u = SY["scale"]
    bad = gc.rounded(v64)
    for m in range(len(SY["modes"])):      # term 4 m + 1: the u x u block of every pixel as the rotated frame made it
        blocks = torch.from_numpy(bad[4 * m + 1]).reshape(N, C, H, u, W, u)
        bad[4 * m + 1] = torch.rot90(blocks, 1, [3, 5]).reshape(N, C, H * u, W * u).numpy()
    _fails(bad, v64, "sub-pixel block of rotation 1 not rotated back")


def test_swapped_taps_c_and_d_are_caught(monkeypatch):
    (x, v64, _), = gc.forward_case(SY, (2, 3, 5, 7))
    for letter in SY["modes"].upper():
        K, (a, b, c, d) = network.TAPS[letter]
        monkeypatch.setitem(network.TAPS, letter, (K, (a, b, d, c)))
    swapped = gc.terms(gc.nets(SY)[1], x, SY["modes"], 1, torch.float64).numpy()
    monkeypatch.undo()
    assert np.array_equal(gc.terms(gc.nets(SY)[1], x, SY["modes"], 1, torch.float64).numpy(), v64)
    _fails(gc.rounded(swapped), v64, "taps c and d swapped")
