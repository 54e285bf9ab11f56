"""The fused network forward on the GPU (-m gpu): mulut_net_table / _pass / _stage through NetEngine against the reference-made
fixtures (tests/golden/transfer_fixtures.npz, net_fixtures.npz), against the torch path of the parent tree on shapes and models the
fixtures do not have, through the deployed LUT engine bit for bit, and on side streams and in a captured graph.

The bar and where it comes from: tests/net_cases.py.  A share is taken over all the values of a kind that a model has (see
tests/test_net_cpu.py)."""
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import net_cases as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    from mulut_amd.net_engine import NetEngine
    made = {name: NetEngine(nc.model(name)) for name in nc.MODELS}
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def transfer_fx():
    return np.load(os.path.join(GOLDEN, "transfer_fixtures.npz"))


# ---------------------------------------------------------------------------------------------------------------- 1. grid form
def test_tables_of_both_fixture_models(engines, transfer_fx):
    """All six tables of the shipped model and the three of the tiny one against the rows the reference's network produced."""
    fx = transfer_fx
    for name, cfg in nc.MODELS.items():
        got, want = [], []
        for s in range(1, cfg["stages"] + 1):
            for m in cfg["modes"]:
                t = engines[name].table(s, m, 4)
                assert t.dtype == torch.int8 and tuple(t.shape) == tuple(fx["%s/s%d_%s/shape" % (name, s, m)])
                got.append(t.cpu().numpy().reshape(t.shape[0], -1)[fx["idx"]].ravel())
                want.append(fx["%s/s%d_%s/rows" % (name, s, m)].ravel())
                nc.meets(got[-1], want[-1], nc.BAR, "%s s%d_%s" % (name, s, m))      # (2048 rows of a table: the bar of test_transfer_cpu.py)
        nc.meets(np.concatenate(got), np.concatenate(want), nc.BAR, name + " tables")
    # a whole-module checkpoint as network.load_checkpoint rebuilds it is walked like a fresh SRNets
    from mulut_amd import network
    from mulut_amd.net_engine import NetEngine
    eng = NetEngine(network.load_checkpoint(os.path.join(GOLDEN, "Model_200000.pth")))
    assert (eng.stages, eng.modes, eng.scale) == (2, "sdy", 4) and torch.equal(eng.table(2, "d", 4), engines["shipped"].table(2, "d", 4))
    eng.close()


WIDE = dict(nf=24, scale=2, modes="sdyeho", stages=2, seed=5)


@pytest.fixture(scope="module")
def wide():
    from mulut_amd.net_engine import NetEngine
    net = nc.seeded_model(**WIDE)
    eng = NetEngine(net)
    yield net.cuda(), eng
    eng.close()


def test_tables_at_intervals_5_and_6_and_of_a_wide_model(engines, wide):
    """Whole tables against transfer_one of the torch path on the GPU: the shipped model at intervals 5 and 6 (6,561 and 625 rows: a
    tail of 1 and of 17 rows past a 32-row tile), a seeded sdyeho model of nf 24 at every interval."""
    from mulut_amd import transfer_to_lut as T
    dev = torch.device("cuda")
    shipped = nc.model("shipped").cuda()
    for name, net, eng, cfg, intervals in (("shipped", shipped, engines["shipped"], nc.MODELS["shipped"], (5, 6)), ("wide", wide[0], wide[1], WIDE, (4, 5, 6))):
        got, want = [], []
        for interval in intervals:
            opt = SimpleNamespace(interval=interval)
            for s in range(1, cfg["stages"] + 1):
                for m in cfg["modes"]:
                    t = eng.table(s, m, interval).cpu().numpy()
                    ref = T.transfer_one(net, opt, s, m, dev, chunks=4)
                    assert t.shape == ref.shape and t.shape[0] == ((256 >> interval) + 1) ** 4
                    got.append(t.ravel())
                    want.append(ref.ravel())
        nc.meets(np.concatenate(got), np.concatenate(want), nc.BAR, name + " tables at intervals %r" % (intervals,))
    nc.model("shipped").cpu()


# ------------------------------------------------------------------------------------------------------- 2. pass and stage forms
@pytest.mark.parametrize("name", sorted(nc.MODELS))
def test_every_fixture_case(engines, name):
    """Per-pass arrays, each stage on the reference's own input bytes, and the cascade on its own bytes."""
    fx, cfg, eng = nc.fixture(), nc.MODELS[name], engines[name]
    S, M = cfg["stages"], len(cfg["modes"])
    kinds = {k: ([], []) for k in ("passes", "stages", "cascade")}
    for c in nc.cases(name):
        x = torch.from_numpy(fx["%s/%s/x" % (name, c)]).cuda()
        kinds["cascade"][0].append(eng.predict(x).cpu().numpy().ravel())
        kinds["cascade"][1].append(fx["%s/%s/s%d/out" % (name, c, S)].ravel())
        for s in range(1, S + 1):
            xin = x if s == 1 else torch.from_numpy(fx["%s/%s/s%d/out" % (name, c, s - 1)]).cuda()
            want_p = fx["%s/%s/s%d/pass" % (name, c, s)]
            got_p = torch.stack([eng.pass_(s, m, r, xin) for m in cfg["modes"] for r in range(4)]).cpu().numpy()
            out = eng.stage(s, xin).cpu().numpy()
            # the stage form is the pass form summed: exactly, whatever the passes are
            assert np.array_equal(out, nc.epilogue(got_p, s == S)), (name, c, s)
            kinds["passes"][0].append(got_p.ravel())
            kinds["passes"][1].append(want_p.ravel())
            kinds["stages"][0].append(out.ravel())
            kinds["stages"][1].append(fx["%s/%s/s%d/out" % (name, c, s)].ravel())
    for kind, cap in (("passes", nc.BAR), ("stages", 4 * M * nc.BAR), ("cascade", S * 4 * M * nc.BAR)):
        nc.meets(np.concatenate(kinds[kind][0]), np.concatenate(kinds[kind][1]), cap, "%s %s" % (name, kind), by_one=kind != "cascade")


SEEDED = [dict(nf=8, scale=3, modes="sd", stages=2, seed=1), dict(nf=64, scale=4, modes="eho", stages=1, seed=2), WIDE,
          dict(nf=33, scale=1, modes="y", stages=2, seed=3)]
SHAPES = [(2, 3, 33, 65), (1, 1, 65, 33), (1, 3, 1, 1), (1, 1, 2, 5)]


@pytest.mark.parametrize("cfg", SEEDED, ids=lambda c: "nf%d_x%d_%s_%d" % (c["nf"], c["scale"], c["modes"], c["stages"]))
def test_seeded_models_against_the_torch_path(cfg, wide):
    """nf 8, 24, 33 and 64 (one and two feature tiles, padded and full), u 1 to 4, one to six patterns, one and two stages, against
    the restatement of net_cases.py run through torch on the GPU."""
    from mulut_amd.net_engine import NetEngine
    if cfg is WIDE:
        net, eng = wide
    else:
        net = nc.seeded_model(**cfg)
        eng = NetEngine(net)
        net = net.cuda()
    S, M = cfg["stages"], len(cfg["modes"])
    assert eng.modes == cfg["modes"] and eng.stages == S and eng.scale == cfg["scale"]
    rng = np.random.default_rng(cfg["seed"])
    kinds = {k: ([], []) for k in ("passes", "stages")}
    for shape in SHAPES:
        x = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).cuda()
        for s, (want_p, want_out) in enumerate(nc.predict_valid(net, x, cfg["modes"], S), 1):
            got_p = torch.stack([eng.pass_(s, m, r, x) for m in cfg["modes"] for r in range(4)])
            got_out = eng.stage(s, x)
            assert np.array_equal(got_out.cpu().numpy(), nc.epilogue(got_p.cpu().numpy(), s == S))
            kinds["passes"][0].append(got_p.cpu().numpy().ravel())
            kinds["passes"][1].append(want_p.cpu().numpy().ravel())
            kinds["stages"][0].append(got_out.cpu().numpy().ravel())
            kinds["stages"][1].append(want_out.cpu().numpy().ravel())
            x = want_out      # every stage is fed the torch path's bytes
    nc.meets(np.concatenate(kinds["passes"][0]), np.concatenate(kinds["passes"][1]), nc.BAR, "passes")
    if M >= 2:
        nc.meets(np.concatenate(kinds["stages"][0]), np.concatenate(kinds["stages"][1]), 4 * M * nc.BAR, "stages")
    else:      # one pattern: a pass value off by one can move pred / M by one, still no further
        worst, share = nc.off(np.concatenate(kinds["stages"][0]), np.concatenate(kinds["stages"][1]))
        assert worst <= 1 and share <= 4 * M * nc.BAR
    if cfg is not WIDE:
        eng.close()


def test_units_that_cannot_run_are_refused():
    from mulut_amd import MuLUTError, network
    from mulut_amd.net_engine import NetEngine
    net = nc.seeded_model(nf=8, scale=2, modes="s", stages=1, seed=0)
    net.s1_s.model = network.MuLUTUnit("2x2", 8, upscale=2, dense=False)
    with pytest.raises(MuLUTError, match="dense"):
        NetEngine(net)
    with pytest.raises(MuLUTError):
        NetEngine(network.SRNets(nf=65, scale=2, modes=["s"], stages=1))
    eng = NetEngine(nc.model("tiny"))
    x = torch.zeros((1, 1, 4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(MuLUTError):
        eng.pass_(1, "s", 4, x)
    with pytest.raises(MuLUTError):
        eng.table(1, "s", 3)
    with pytest.raises(ValueError):
        eng.pass_(1, "e", 0, x)
    with pytest.raises(TypeError):
        eng.stage(1, x.float())
    eng.close()


# --------------------------------------------------------------------------------------------- 3. predict and validation on Set5
@pytest.fixture(scope="module")
def set5_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("bench")
    shutil.copytree(os.path.join(GOLDEN, "Set5", "HR"), str(root / "Set5" / "HR"))
    shutil.copytree(os.path.join(GOLDEN, "Set5", "LR_bicubic"), str(root / "Set5" / "LR_bicubic"))
    return str(root)


def test_predict_and_validation_on_set5(engines, set5_dir, tmp_path):
    from PIL import Image
    from mulut_amd import metrics
    from mulut_amd.net_val import net_valid_steps
    fx, eng, cfg = nc.fixture(), engines["shipped"], nc.MODELS["shipped"]
    opt = SimpleNamespace(valDir=set5_dir, valoutDir=str(tmp_path / "val"), scale=4, debug=True)
    lines = []
    res = net_valid_steps(eng, opt, 200000, lines.append)
    assert list(res) == ["Set5"] and len(res["Set5"]) == 5 and len(lines) == 1
    net = nc.model("shipped").cuda()
    got, want, psnrs = [], [], []
    for k, name in enumerate(nc.SET5):
        lr = np.array(Image.open(os.path.join(GOLDEN, "Set5", "LR_bicubic", "X4", name + ".png")))
        hr = np.array(Image.open(os.path.join(GOLDEN, "Set5", "HR", name + ".png")))
        x = torch.from_numpy(np.ascontiguousarray(lr.transpose(2, 0, 1)[None])).cuda()
        pred = eng.predict(x)[0].permute(1, 2, 0).contiguous().cpu().numpy()
        # the file of the validation holds these bytes; below iteration 10000 only are input and gt saved
        assert np.array_equal(np.array(Image.open(os.path.join(opt.valoutDir, "Set5", name + "_net.png"))), pred)
        assert not os.path.exists(os.path.join(opt.valoutDir, "Set5", name + "_gt.png"))
        got.append(pred.ravel())
        want.append(nc.predict_valid(net, x, cfg["modes"], cfg["stages"])[-1][1][0].permute(1, 2, 0).cpu().numpy().ravel())
        psnrs.append(metrics.psnr(metrics.rgb2ycbcr(pred)[:, :, 0], metrics.rgb2ycbcr(hr)[:, :, 0], 4))
        assert psnrs[-1] == res["Set5"][k]
        assert abs(psnrs[-1] - float(fx["set5/%s/psnr" % name])) <= 5e-3, name
    nc.model("shipped").cpu()
    nc.meets(np.concatenate(got), np.concatenate(want), cfg["stages"] * 4 * len(cfg["modes"]) * nc.BAR, "Set5 bytes", by_one=False)
    mean = np.mean(np.asarray(psnrs, dtype=np.float64))
    assert lines[0] == 'Iter {} | Dataset {} | AVG Val PSNR: {}'.format(200000, "Set5", mean)
    print(lines[0])
    assert abs(mean - np.mean([float(fx["set5/%s/psnr" % n]) for n in nc.SET5])) <= 5e-3
    assert abs(mean - 30.607945948346618) <= 5e-3 and float(fx["set5/train_log_psnr"]) == 30.607945948346618
    # an early iteration also writes the input and the ground truth
    opt.valoutDir = str(tmp_path / "early")
    net_valid_steps(eng, opt, 1, lines.append)
    assert sorted(os.listdir(os.path.join(opt.valoutDir, "Set5")))[:3] == ["baby_gt.png", "baby_input.png", "baby_net.png"]


# -------------------------------------------------------------------------------- 4. self-consistency through the deployed engine
def test_fused_tables_in_the_lut_engine_give_the_network_bytes(engines, tmp_path):
    """`--fused` writes the tables; a MuLUTEngine holding them and the NetEngine then agree bit for bit on an image of grid values
    (0, 16, ..., 240: there a site is an exact look-up of a row that the same site body produced; 255 is interpolated by the LUT
    engine), at every stage."""
    from mulut_amd import MuLUTEngine, transfer_to_lut as T
    from mulut_amd.engine import LAYOUT_CHW
    exp = tmp_path / "exp"
    exp.mkdir()
    shutil.copyfile(os.path.join(GOLDEN, "Model_200000.pth"), str(exp / "Model_200000.pth"))
    tabs = T.main(["--stages", "2", "--modes", "sdy", "-e", str(exp), "--fused"])
    plain = T.TransferOptions().parse(["--stages", "2", "--modes", "sdy", "-e", str(exp)])
    lut = MuLUTEngine(0).configure(2, "sdy", 4, 4)
    for s in (1, 2):
        for m in "sdy":
            key = "s%d_%s" % (s, m)
            on_disk = np.load(os.path.join(str(exp), T.lut_file_name(plain, s, m)))
            assert on_disk.dtype == np.int8 and on_disk.shape == (83521, 1, 4 if s == 2 else 1, 4 if s == 2 else 1)
            assert np.array_equal(on_disk, tabs[key]) and np.array_equal(on_disk, engines["shipped"].table(s, m, 4).cpu().numpy())
            lut.set_lut(s, m, on_disk)
    rng = np.random.default_rng(9)
    for shape in ((2, 3, 33, 65), (1, 1, 65, 33), (1, 3, 1, 1)):
        x = torch.from_numpy((rng.integers(0, 16, shape) * 16).astype(np.uint8)).cuda()
        for s in (1, 2):
            a = lut.stage(s, x, layout=LAYOUT_CHW)
            b = engines["shipped"].stage(s, x)
            assert a.shape == b.shape and torch.equal(a, b), (shape, s, int((a != b).sum()))
    lut.close()


# ---------------------------------------------------------------------------------------------------- 5. streams and graphs
def test_calls_on_a_non_blocking_side_stream(engines):
    eng = engines["shipped"]
    x = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (1, 3, 33, 65), dtype=np.uint8)).cuda()
    want = (eng.table(2, "y", 4), eng.pass_(2, "d", 3, x), eng.stage(1, x), eng.predict(x))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()      # (torch's streams are non-blocking: no implicit order with the default stream)
    with torch.cuda.stream(side):
        got = (eng.table(2, "y", 4), eng.pass_(2, "d", 3, x), eng.stage(1, x), eng.predict(x))
    side.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_a_captured_stage_replays_on_a_rewritten_input(engines):
    eng = engines["shipped"]
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.integers(0, 256, (1, 3, 33, 65), dtype=np.uint8)).cuda()
    out = torch.zeros((1, 3, 132, 260), dtype=torch.uint8, device="cuda")
    first = eng.stage(2, x).clone()      # the warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.stage(2, x, out=out)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    x.copy_(torch.from_numpy(rng.integers(0, 256, (1, 3, 33, 65), dtype=np.uint8)))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    direct = eng.stage(2, x)
    assert torch.equal(out, direct) and not torch.equal(out, first)
