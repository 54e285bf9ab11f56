"""The list form of the cascade on the GPU (-m gpu): mulut_net_plan_* through NetEngine.plan, bit for bit against NetEngine.predict of
each image alone, permuted to HWC -- no tolerance anywhere -- and the resident validation of network training built on it
(net_val.resident_net_valid_steps, train_model --valResident) against the host loop.  Lists, models and pools: tests/net_list_cases.py."""
import os
import re
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN

import net_cases as nc
import net_list_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    return {name: nc.seeded_model(**cfg) for name, cfg in L.MODELS.items()}


@pytest.fixture(scope="module")
def engines(models):
    from mulut_amd.net_engine import NetEngine
    made = {name: NetEngine(net) for name, net in models.items()}
    yield made
    for e in made.values():
        e.close()


def predict_hwc(eng, im):
    """NetEngine.predict of one H x W x C image alone, as H*scale x W*scale x C bytes on the host: the definition of an item's result."""
    x = torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[None])).cuda()
    return eng.predict(x)[0].permute(1, 2, 0).contiguous().cpu().numpy()


_want = {}


def wanted(name, eng, pools, key):
    """The per-image results of a (model, list), computed once and shared."""
    if (name, key) not in _want:
        _want[name, key] = [predict_hwc(eng, im) for im in pools.images]
    return _want[name, key]


def same(pools, out_pool, want, what):
    for k, w in enumerate(want):
        got = pools.result(out_pool, k)
        assert got.shape == w.shape and np.array_equal(got, w), "%s: item %d (%r): %d bytes differ" % (what, k, pools.shapes[k], int((got != w).sum()))
    outside = pools.outside(out_pool)
    assert (outside == pools.GUARD).all(), "%s: %d bytes outside the items' ranges were written" % (what, int((outside != pools.GUARD).sum()))


def run_list(eng, pools, plan=None):
    """One run of a plan over the pools; the output pool starts as guard bytes.  Returns it on the host."""
    own = plan is None
    plan = eng.plan(pools.items(), ch=pools.ch) if own else plan
    out = torch.from_numpy(pools.fresh_out()).cuda()
    plan.run(torch.from_numpy(pools.in_pool).cuda(), out)
    got = out.cpu().numpy()
    if own:
        plan.close()
    return got


# ------------------------------------------------------------------------------------------------------------ 1. one mixed list
@pytest.mark.parametrize("name", sorted(L.MODELS))
def test_mixed_list_is_predict_per_image(engines, name):
    """1 x 1, 2 x 3, 5 x 7, 6 x 7, 43 x 1, 11 x 12, 1 x 43 in one list, three channels: partial workgroups, plane boundaries inside a
    workgroup, images smaller than the pad.  Two stages at x4, one at x2, three of e, h, o at x3; nf 8, 33 and 64."""
    eng, cfg = engines[name], L.MODELS[name]
    assert (eng.stages, eng.scale) == (cfg["stages"], cfg["scale"])
    pools = L.Pools(L.MIXED, 3, cfg["scale"], seed=1)
    same(pools, run_list(eng, pools), wanted(name, eng, pools, "mixed"), name)


# --------------------------------------------------------------------------------------------------------------- 2. pool layout
def test_pool_layout_out_of_order_odd_offsets_guard_bands(engines):
    """The slots of the output pool lie in another order than the inputs, every offset is odd, a guard band of a known byte lies
    around every slot of both pools: every item lands in its slot and no byte outside the items' ranges is written.  The pools'
    base addresses are moved by one byte too (a view from element 1)."""
    name = "x4_sdy_nf8"
    eng = engines[name]
    pools = L.Pools(L.MIXED, 3, 4, seed=1)
    assert all(o % 2 == 1 for o in pools.in_off + pools.out_off)
    assert np.argsort(pools.in_off).tolist() == list(range(len(L.MIXED))) and np.argsort(pools.out_off).tolist() == list(range(len(L.MIXED)))[::-1]
    want = wanted(name, eng, pools, "mixed")
    plan = eng.plan(pools.items(), ch=3)
    for shift in (0, 1):
        tin = torch.full((pools.in_bytes + 1,), 0x11, dtype=torch.uint8, device="cuda")[shift:shift + pools.in_bytes]
        tout = torch.full((pools.out_bytes + 1,), pools.GUARD, dtype=torch.uint8, device="cuda")[shift:shift + pools.out_bytes]
        assert tin.data_ptr() % 2 == shift
        tin.copy_(torch.from_numpy(pools.in_pool))
        plan.run(tin, tout)
        same(pools, tout.cpu().numpy(), want, "shift %d" % shift)
    with pytest.raises(ValueError):
        plan.run(tin[:-1], tout)
    with pytest.raises(ValueError):
        plan.run(tin, tout[:-1])
    plan.close()
    from mulut_amd.engine import MuLUTError
    with pytest.raises(MuLUTError):
        plan.run(tin, tout)
    # overlapping result ranges are refused through the engine too
    items = pools.items()
    items[1] = (items[1][0], items[0][1] + 1) + items[1][2:]
    with pytest.raises(MuLUTError):
        eng.plan(items, ch=3)


# -------------------------------------------------------------------------------------------------------------------- 3. ch = 1
@pytest.mark.parametrize("name", ["x3_eho_nf8", "x4_sdy_nf33", "x2_one_stage_nf8"])
def test_single_channel_list(engines, name):
    eng = engines[name]
    pools = L.Pools(L.MIXED, 1, L.MODELS[name]["scale"], seed=2)
    same(pools, run_list(eng, pools), wanted(name, eng, pools, "grey"), name)


# ---------------------------------------------------------------------------------------------------------------- 4. 328 items
@pytest.mark.parametrize("name", ["x4_sdy_nf8", "x3_eho_nf33"])
def test_list_of_328_small_items(engines, name):
    """As many items as the five benchmark sets hold: a map of more than one page of workgroups."""
    eng = engines[name]
    pools = L.Pools(L.MANY, 3, L.MODELS[name]["scale"], seed=3, guard=5)
    assert len(L.tables(L.MANY, 3, eng.stages, eng.scale)[1]) > 512
    # the reference in batches of equal shape (predict takes one): the planes of a batch are independent, as the items of a list are
    want = [None] * len(pools.images)
    for shape in sorted(set(L.MANY)):
        idx = [k for k, s in enumerate(L.MANY) if s == shape]
        x = torch.from_numpy(np.ascontiguousarray(np.stack([pools.images[k] for k in idx]).transpose(0, 3, 1, 2))).cuda()
        y = eng.predict(x).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        for j, k in enumerate(idx):
            want[k] = y[j]
    assert np.array_equal(want[7], predict_hwc(eng, pools.images[7]))
    same(pools, run_list(eng, pools), want, name)


# --------------------------------------------------------------------------------------------------------------- 5. the fixtures
@pytest.mark.parametrize("name", sorted(nc.MODELS))
def test_fixture_cases_as_a_list(name):
    """The inputs of golden/net_fixtures.npz, every image of every case, as one list per channel count: bit for bit predict per image,
    and against the reference's own bytes under the cascade's bar of tests/net_cases.py."""
    from mulut_amd.net_engine import NetEngine
    fx, cfg = nc.fixture(), nc.MODELS[name]
    eng = NetEngine(nc.model(name))
    got_all, ref_all = [], []
    for ch in (1, 3):
        images, refs = [], []
        for c in nc.cases(name):
            x, out = fx["%s/%s/x" % (name, c)], fx["%s/%s/s%d/out" % (name, c, cfg["stages"])]
            if x.shape[1] == ch:
                images += [np.ascontiguousarray(x[n].transpose(1, 2, 0)) for n in range(x.shape[0])]
                refs += [out[n].transpose(1, 2, 0) for n in range(x.shape[0])]
        assert images
        pools = L.Pools([im.shape[:2] for im in images], ch, cfg["scale"])
        pools.images = images
        for k, im in enumerate(images):
            pools.in_pool[pools.in_off[k]:pools.in_off[k] + im.size] = im.reshape(-1)
        out = run_list(eng, pools)
        same(pools, out, [predict_hwc(eng, im) for im in images], "%s ch %d" % (name, ch))
        got_all += [pools.result(out, k).ravel() for k in range(len(images))]
        ref_all += [r.ravel() for r in refs]
    nc.meets(np.concatenate(got_all), np.concatenate(ref_all), cfg["stages"] * 4 * len(cfg["modes"]) * nc.BAR, name + " list against the fixture", by_one=False)
    eng.close()


# ----------------------------------------------------------------------------------------------------------- 6. weights refreshed
def test_plan_sees_refreshed_weights():
    from mulut_amd.net_engine import NetEngine
    net = nc.seeded_model(nf=8, scale=4, modes="sd", stages=2, seed=21).cuda()
    eng = NetEngine(net)
    pools = L.Pools(L.MIXED, 3, 4, seed=4)
    plan = eng.plan(pools.items())
    before = run_list(eng, pools, plan)
    same(pools, before, [predict_hwc(eng, im) for im in pools.images], "before")
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn(p.shape, generator=g, device="cuda") * 0.1)
    assert np.array_equal(run_list(eng, pools, plan), before)      # the units hold what they were given, until load_weights
    eng.load_weights(net)
    after = run_list(eng, pools, plan)
    same(pools, after, [predict_hwc(eng, im) for im in pools.images], "after")
    assert not np.array_equal(after, before)
    plan.close()
    eng.close()


# --------------------------------------------------------------------------------------------------- 7., 8. a side stream, a graph
def test_run_on_a_side_stream(engines):
    name = "x3_eho_nf8"
    eng = engines[name]
    pools = L.Pools(L.MIXED, 3, 3, seed=1)
    want = wanted(name, eng, pools, "mixed")
    plan = eng.plan(pools.items())
    tin, out = torch.from_numpy(pools.in_pool).cuda(), torch.from_numpy(pools.fresh_out()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        plan.run(tin, out)
    side.synchronize()
    same(pools, out.cpu().numpy(), want, "side stream")
    plan.close()


def test_run_in_a_captured_graph_replayed_on_new_input(engines):
    """A run is `stages` launches and nothing else, so it captures; the replay reads the input pool as it is then."""
    name = "x4_sdy_nf33"
    eng = engines[name]
    pools, other = L.Pools(L.MIXED, 3, 4, seed=1), L.Pools(L.MIXED, 3, 4, seed=6)
    plan = eng.plan(pools.items())
    tin, out = torch.from_numpy(pools.in_pool).cuda(), torch.from_numpy(pools.fresh_out()).cuda()
    plan.run(tin, out)      # the warm-up
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    same(pools, first, wanted(name, eng, pools, "mixed"), "direct")
    out.fill_(pools.GUARD)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run(tin, out)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), first)
    tin.copy_(torch.from_numpy(other.in_pool))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    again = out.cpu().numpy()
    same(other, again, [predict_hwc(eng, im) for im in other.images], "replay")
    assert not np.array_equal(again, first)
    del graph
    plan.close()


# ---------------------------------------------------------------------------------------------------------------- 9. two plans
def test_two_plans_on_one_engine(engines):
    name = "x4_sdy_nf8"
    eng = engines[name]
    a, b = L.Pools(L.MIXED, 3, 4, seed=1), L.Pools(L.MIXED[::-1] + [(9, 9)], 3, 4, seed=7)
    pa, pb = eng.plan(a.items()), eng.plan(b.items())
    ia, ib = torch.from_numpy(a.in_pool).cuda(), torch.from_numpy(b.in_pool).cuda()
    oa, ob = torch.from_numpy(a.fresh_out()).cuda(), torch.from_numpy(b.fresh_out()).cuda()
    for _ in range(2):      # interleaved on one stream
        pa.run(ia, oa)
        pb.run(ib, ob)
    same(a, oa.cpu().numpy(), wanted(name, eng, a, "mixed"), "plan a")
    same(b, ob.cpu().numpy(), [predict_hwc(eng, im) for im in b.images], "plan b")
    pa.close()
    pb.close()


# ------------------------------------------------------------------------------------------------- 10. the resident validation
def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


@pytest.fixture(scope="module")
def bench_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("bench")
    shutil.copytree(os.path.join(GOLDEN, "Set5", "HR"), str(root / "Set5" / "HR"))
    shutil.copytree(os.path.join(GOLDEN, "Set5", "LR_bicubic"), str(root / "Set5" / "LR_bicubic"))
    return str(root)


def _opt(val, out, **kw):
    base = dict(valDir=val, valoutDir=str(out), scale=4, debug=True, valSave="every", totalIter=100, valStep=10)
    base.update(kw)
    return SimpleNamespace(**base)


def _tree(root):
    """{relative path: file bytes} of everything under `root`."""
    out = {}
    for d, _, fs in os.walk(str(root)):
        for fn in fs:
            with open(os.path.join(d, fn), "rb") as f:
                out[os.path.relpath(os.path.join(d, fn), str(root))] = f.read()
    return out


@pytest.fixture(scope="module")
def val_points(tmp_path_factory, bench_dir):
    """net_valid_steps and resident_net_valid_steps (--valSave every) side by side on Set5 with the nf-8 x4 model, at iterations 7 and
    9 with the weights changed between: (lines, results, tree) of each path at each point."""
    from mulut_amd.net_engine import NetEngine
    from mulut_amd.net_val import NetValSet, net_valid_steps, resident_net_valid_steps
    tmp = tmp_path_factory.mktemp("val")
    net = nc.seeded_model(nf=8, scale=4, modes="sdy", stages=2, seed=31).cuda()
    eng = NetEngine(net)
    host_opt, res_opt = _opt(bench_dir, tmp / "host"), _opt(bench_dir, tmp / "resident")
    vset = NetValSet(res_opt, workers=2)
    assert vset.lr_f32 is None and vset.nbytes == 2 * vset.gt_bytes + vset.lr_bytes and [s["name"] for s in vset.sets] == ["Set5"]
    points = []
    for it in (7, 9):
        a_lines, b_lines = [], []
        a = net_valid_steps(eng, host_opt, it, a_lines.append)
        b = resident_net_valid_steps(eng, vset, res_opt, it, b_lines.append)
        vset.join()
        points.append(((a_lines, a, _tree(tmp / "host")), (b_lines, b, _tree(tmp / "resident"))))
        g = torch.Generator(device="cuda").manual_seed(it)
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn(p.shape, generator=g, device="cuda") * 0.05)
        eng.load_weights(net)
    vset.close()
    eng.close()
    return points


def test_resident_validation_writes_the_host_loops_files(val_points):
    """--valSave every: valoutDir holds the same names and the same bytes as the host loop leaves, at both points; the second
    point's results differ from the first's."""
    for (_, _, host), (_, _, res) in val_points:
        assert sorted(host) == sorted(res) and len(host) == 15
        assert sorted(os.path.basename(k) for k in host if "baby" in k) == ["baby_gt.png", "baby_input.png", "baby_net.png"]
        assert all(host[k] == res[k] for k in host), [k for k in host if host[k] != res[k]]
    first, second = val_points[0][1][2], val_points[1][1][2]
    assert all((first[k] != second[k]) == k.endswith("_net.png") for k in first)


def test_resident_validation_lines_and_arrays_are_the_host_loops(val_points):
    """Equal log lines and equal returned arrays, as doubles: the resident point scores the bytes it read back with metrics.psnr,
    the host loop's own float32 arithmetic (mulut_eval_finish, float64 behind the mean, prints other digits from the seventh on)."""
    for (a_lines, a, _), (b_lines, b, _) in val_points:
        print(a_lines, b_lines)
        assert list(a) == list(b) == ["Set5"] and b["Set5"].dtype == a["Set5"].dtype == np.float64 and b["Set5"].shape == (5,)
        assert bits(a["Set5"]).tolist() == bits(b["Set5"]).tolist()
        assert a_lines == b_lines and len(a_lines) == 1
    assert val_points[0][0][0] != val_points[1][0][0]


def test_val_save_last_and_never_and_the_fall_back(tmp_path, bench_dir, val_points):
    from mulut_amd.ft_val import ValidationSetTooLarge
    from mulut_amd.net_engine import NetEngine
    from mulut_amd.net_val import NetValSet, resident_net_valid_steps
    eng = NetEngine(nc.seeded_model(nf=8, scale=4, modes="sdy", stages=2, seed=31))
    want = val_points[0][1]      # the same weights as the first point
    for save, its, files in (("last", (2, 4), 15), ("never", (2, 4), 0)):
        opt = _opt(bench_dir, tmp_path / save, valSave=save, totalIter=5, valStep=2)
        vset = NetValSet(opt, workers=2)
        for it in its:
            lines = []
            res = resident_net_valid_steps(eng, vset, opt, it, lines.append)
            vset.join()
            assert bits(res["Set5"]).tolist() == bits(want[1]["Set5"]).tolist()
            tree = _tree(tmp_path / save)
            assert len(tree) == (files if it == its[-1] else 0), (save, it, sorted(tree))
        if files:
            assert tree == want[2]
        vset.close()
    # a set that does not fit: refused before anything is allocated, with the sizes
    with pytest.raises(ValidationSetTooLarge) as e:
        NetValSet(_opt(bench_dir, tmp_path / "small"), max_bytes=1000)
    assert e.value.limit == 1000 and e.value.nbytes > 1000
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 11. the driver
def _drive(exp, bench, extra=()):
    from mulut_amd import train_model
    from mulut_amd.options import TrainOptions
    opt = TrainOptions().parse(["-e", str(exp), "--nf", "8", "--stages", "2", "--modes", "sd", "--scale", "4", "--batchSize", "4", "--cropSize", "12",
                                "--trainDir", os.path.join(GOLDEN, "Set5"), "--valDir", bench, "--totalIter", "4", "--displayStep", "1",
                                "--saveStep", "100", "--valStep", "2", "--seed", "3", "--deterministic"] + list(extra))
    lines = []
    _, losses = train_model.train(opt, lines.append)
    lines = [re.sub(r"[dr]T:[0-9.eE+-]+", "T:*", ln).replace(str(exp), "EXP") for ln in lines]
    return opt, lines, losses


@pytest.fixture(scope="module")
def drives(tmp_path_factory, bench_dir):
    tmp = tmp_path_factory.mktemp("drive")
    host = _drive(tmp / "host", bench_dir)
    res = _drive(tmp / "resident", bench_dir, ["--valResident", "--valWorkers", "2"])
    return host, res


def test_driver_with_the_resident_validation_trains_and_writes_the_same(drives):
    """train_model.train, 4 iterations, validation at 2 and 4: the losses, every line but the validation lines, and valoutDir do not
    depend on --valResident.  Both runs are --deterministic --seed: the default backward adds the earlier stage's input gradient with
    float atomics, so two runs of it end in weights that differ in their last bits and may differ in a byte of a result."""
    (h_opt, h_lines, h_losses), (r_opt, r_lines, r_losses) = drives
    assert h_losses == r_losses and len(h_losses) == 4
    val = lambda lines: [ln for ln in lines if "AVG Val PSNR" in ln]      # noqa: E731
    assert len(val(h_lines)) == len(val(r_lines)) == 2 and r_lines[-1] == "Complete"
    assert [ln for ln in h_lines if ln not in val(h_lines)] == [ln for ln in r_lines if ln not in val(r_lines)]
    assert [ln.split("PSNR: ")[0] for ln in val(h_lines)] == [ln.split("PSNR: ")[0] for ln in val(r_lines)]
    h_tree, r_tree = _tree(h_opt.valoutDir), _tree(r_opt.valoutDir)
    assert len(h_tree) == 15 and h_tree == r_tree


def test_driver_with_the_resident_validation_logs_the_same_lines(drives):
    """Equal log lines, the validation lines included (the step times apart)."""
    (_, h_lines, _), (_, r_lines, _) = drives
    print([ln for ln in h_lines if "AVG Val PSNR" in ln], [ln for ln in r_lines if "AVG Val PSNR" in ln])
    assert h_lines == r_lines


def test_driver_falls_back_when_the_set_does_not_fit(tmp_path, bench_dir, monkeypatch):
    from mulut_amd import train_model
    from mulut_amd.ft_val import ValidationSetTooLarge
    opt = SimpleNamespace(expDir="EXP", valWorkers=2)

    def too_large(*a, **kw):
        raise ValidationSetTooLarge(10, 5)
    monkeypatch.setattr(train_model, "NetValSet", too_large)
    lines = []
    assert train_model.resident_val_set(opt, lines.append) is None
    assert lines == ["EXP | validation set of 10 bytes exceeds half the free device memory (5): validation runs on the host loop"]


def test_transfer_validates_from_the_resident_set(tmp_path, bench_dir, capsys):
    """transfer_to_lut --fused --valDir --valResident: the single point through the resident path, its files those of the host loop."""
    from mulut_amd import transfer_to_lut as T
    net = nc.seeded_model(nf=8, scale=4, modes="sd", stages=2, seed=41)
    trees = {}
    for name, extra in (("host", []), ("resident", ["--valResident"])):
        exp = tmp_path / name
        os.makedirs(str(exp))
        torch.save(net, os.path.join(str(exp), "Model_000012.pth"))
        T.main(["--stages", "2", "--modes", "sd", "--scale", "4", "--nf", "8", "-e", str(exp), "--loadIter", "12", "--fused", "--valDir", bench_dir, "--debug"] + extra)
        trees[name] = _tree(exp / "val")
        assert sum("AVG Val PSNR" in ln for ln in capsys.readouterr().out.splitlines()) == 1
    assert len(trees["host"]) == 15 and trees["host"] == trees["resident"]
