"""The resident validation of the fine-tune driver on the GPU: the list scorer (mulut_eval_plan_*) held to mulut_eval_y bit for bit,
mulut_ft_val_pack to the torch expression of valid_steps byte for byte, resident_valid_steps / resident_engine_valid_steps to
valid_steps / engine_valid_steps (lines, doubles, files), the fall-back and the driver's flags.  Cases: tests/val_cases.py."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
from PIL import Image

import val_cases as V
from conftest import GOLDEN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import _native, finetune_lut  # noqa: E402


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def stream_ptr(stream=None):
    return ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def eval_y(lib, gt, out, shave):
    """mulut_eval_y's two doubles for one pair of device tensors."""
    H, W = int(gt.shape[0]), int(gt.shape[1])
    n = int(lib.mulut_eval_ws_doubles(H, W))
    ws = torch.empty(n, dtype=torch.float64, device="cuda")
    p, s = ctypes.c_double(), ctypes.c_double()
    assert lib.mulut_eval_y(0, gt.data_ptr(), out.data_ptr(), H, W, shave, ws.data_ptr(), n, ctypes.byref(p), ctypes.byref(s), stream_ptr()) == 0
    return p.value, s.value


class Plan(object):
    def __init__(self, lib, rows, gt_bytes, out_bytes, shave):
        self.lib, self.rows, self.shave = lib, rows, shave
        self.items = V.item_table(rows, gt_bytes, out_bytes)
        self.h = ctypes.c_void_p()
        rc = lib.mulut_eval_plan_create(0, self.items.ctypes.data, len(rows), shave, ctypes.byref(self.h))
        assert rc == 0 and self.h.value, rc
        self.sums = torch.full((len(rows), 2), -7.0, dtype=torch.float64, device="cuda")

    def run(self, gt_pool, out_pool, stream=None):
        assert self.lib.mulut_eval_plan_run(self.h, gt_pool.data_ptr(), out_pool.data_ptr(), self.sums.data_ptr(), stream_ptr(stream)) == 0

    def scores(self):
        """mulut_eval_finish of every item's two sums, after waiting for the device."""
        torch.cuda.synchronize()
        sums, out = self.sums.cpu().numpy(), []
        p, s = ctypes.c_double(), ctypes.c_double()
        for (_, _, H, W), (a, b) in zip(self.rows, sums):
            assert self.lib.mulut_eval_finish(float(a), float(b), H, W, self.shave, ctypes.byref(p), ctypes.byref(s)) == 0
            out.append((p.value, s.value))
        return out

    def close(self):
        assert self.lib.mulut_eval_plan_destroy(self.h) == 0


@pytest.fixture(scope="module")
def pairs():
    return V.list_pairs()


@pytest.fixture(scope="module")
def want(lib, pairs):
    """{(pair index, shave): mulut_eval_y's (PSNR, SSIM)}: computed once, shared, never changed."""
    out = {}
    for i, (_, gt, o) in enumerate(pairs):
        g, d = dev(gt), dev(o)
        for shave in V.SHAVES:
            out[i, shave] = eval_y(lib, g, d, shave)
    return out


@pytest.mark.parametrize("shave", V.SHAVES)
def test_list_scorer_gives_eval_ys_doubles_bit_for_bit(lib, pairs, want, shave):
    """One plan over all the pairs of val_cases.SHAPES, every image at its own (mostly odd) byte offset in either pool; then the same
    items in another order: the same bits per item."""
    names = [n for n, _, _ in pairs]
    assert want[names.index("identical"), shave][0] == float("inf")
    for order in (None, [5, 8, 0, 7, 3, 6, 1, 4, 2]):
        g, o, rows = V.pack_pools(pairs, order)
        assert any(r[0] % 2 for r in rows) and any(r[1] % 2 for r in rows) and any(r[0] % 4 != r[1] % 4 for r in rows)
        plan = Plan(lib, rows, g.size, o.size, shave)
        plan.run(dev(g), dev(o))
        got = plan.scores()
        plan.close()
        for k, i in enumerate(order or range(len(pairs))):
            print(names[i], shave, got[k], want[i, shave])
            assert bits(got[k]).tolist() == bits(want[i, shave]).tolist(), (names[i], shave, got[k], want[i, shave])


def test_list_scorer_on_328_small_items(lib):
    rng = np.random.default_rng(9)
    many = [("p%d" % i, rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), None) for i in range(328)]
    many = [(n, gt, np.clip(gt.astype(np.int32) + rng.integers(-9, 10, gt.shape), 0, 255).astype(np.uint8)) for n, gt, _ in many]
    g, o, rows = V.pack_pools(many)
    plan = Plan(lib, rows, g.size, o.size, 4)
    plan.run(dev(g), dev(o))
    got = plan.scores()
    plan.close()
    ref = [eval_y(lib, dev(gt), dev(out), 4) for _, gt, out in many]
    assert bits(got).tolist() == bits(ref).tolist()


def test_list_scorer_captured_into_a_graph_and_on_a_side_stream(lib, pairs, want):
    """The run launches and nothing else: captured once, replayed after the output pool changed (twice), it scores what the pool
    holds then; and on a non-blocking side stream it runs behind the copy that fills the pool on that stream."""
    small = [p for p in pairs if p[0] != "second_pass"]
    idx = [i for i, p in enumerate(pairs) if p[0] != "second_pass"]
    g, o, rows = V.pack_pools(small)
    gt_pool, out_pool = dev(g), torch.zeros(o.size, dtype=torch.uint8, device="cuda")
    plan = Plan(lib, rows, g.size, o.size, 4)
    side = torch.cuda.Stream()
    host_o = torch.from_numpy(o).pin_memory()
    with torch.cuda.stream(side):                       # (also the warm-up run before the capture)
        out_pool.copy_(host_o, non_blocking=True)
        plan.run(gt_pool, out_pool, side)
    side.synchronize()
    first = plan.scores()
    for k, i in enumerate(idx):
        assert bits(first[k]).tolist() == bits(want[i, 4]).tolist(), pairs[i][0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.run(gt_pool, out_pool, side)
    for turn in (1, 2):
        # the outputs rotated among the items of one shape: (53, 75) holds three pairs
        swapped = list(small)
        same = [k for k, p in enumerate(small) if p[1].shape == (53, 75, 3)]
        for a, b in zip(same, same[turn:] + same[:turn]):
            swapped[a] = (small[a][0], small[a][1], small[b][2])
        _, o2, _ = V.pack_pools(swapped)
        out_pool.copy_(dev(o2))
        plan.sums.fill_(-7.0)
        torch.cuda.synchronize()
        graph.replay()
        got = plan.scores()
        for k, (name, gt, out) in enumerate(swapped):
            assert bits(got[k]).tolist() == bits(eval_y(lib, dev(gt), dev(out), 4)).tolist(), (turn, name)
        assert bits(got).tolist() != bits(first).tolist()
    del graph
    plan.close()


# ------------------------------------------------------------------------------------------------------------ mulut_ft_val_pack
@pytest.mark.parametrize("name", list(V.pack_inputs()))
def test_val_pack_writes_the_bytes_of_valid_steps(lib, name):
    """Against the torch expression of valid_steps, into an output at an odd address with guard bytes on both sides."""
    x = V.pack_inputs()[name]
    _, H, W = x.shape
    pred = dev(x)
    scaled = pred[None] * 255.0
    want = torch.round(torch.clamp(scaled[0].permute(1, 2, 0), 0, 255)).to(torch.uint8).contiguous().cpu().numpy()
    if name.startswith("ties"):
        on = int(((scaled % 1.0) == 0.5).sum())
        print("inputs whose float32 product with 255 is a tie: %d of %d" % (on, scaled.numel()))
        assert on >= 3 * 255
    if name.startswith("bytes"):
        assert np.array_equal(want[:, :, 0].reshape(-1), np.arange(256, dtype=np.uint8))
    n = H * W * 3
    buf = torch.full((17 + n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + 17) % 2 == 1
    assert lib.mulut_ft_val_pack(0, pred.data_ptr(), H, W, buf.data_ptr() + 17, stream_ptr()) == 0
    got = buf.cpu().numpy()
    assert (got[:17] == 0xEE).all() and (got[17 + n:] == 0xEE).all()
    assert np.array_equal(got[17:17 + n].reshape(H, W, 3), want), "%d bytes differ" % int((got[17:17 + n].reshape(H, W, 3) != want).sum())


# ------------------------------------------------------------------------------------------------- the resident validation
def _opt(val, out, **kw):
    base = dict(valDir=val, valoutDir=str(out), scale=4, debug=True, valSave="every", totalIter=100, valStep=10)
    base.update(kw)
    return argparse.Namespace(**base)


def _net(tmp_path, model, modes, interval, shipped):
    from mulut_amd import finetune
    exp = V.write_exp(tmp_path / "exp", modes, interval, shipped)
    return getattr(finetune, model)(exp, 2, list(modes), upscale=4, interval=interval).cuda()


def _same_results(a, b):
    assert list(a) == list(b)
    for ds in a:
        assert a[ds].dtype == b[ds].dtype == np.float64 and a[ds].shape == b[ds].shape
        assert bits(a[ds]).tolist() == bits(b[ds]).tolist(), ds


def _same_files(dir_a, dir_b, files):
    pixels = {}
    for ds, names in files.items():
        want_names = sorted(fn[:-4].split("_")[-1] + "_lutft.png" for fn in names)
        assert sorted(os.listdir(os.path.join(dir_a, ds))) == sorted(os.listdir(os.path.join(dir_b, ds))) == want_names
        for fn in want_names:
            a, b = np.array(Image.open(os.path.join(dir_a, ds, fn))), np.array(Image.open(os.path.join(dir_b, ds, fn)))
            assert a.shape == b.shape and a.dtype == b.dtype == np.uint8 and np.array_equal(a, b), (ds, fn)
            pixels[ds, fn] = a
    return pixels


def _perturb(net):
    g = torch.Generator(device="cuda").manual_seed(3)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn(p.shape, generator=g, device="cuda") * 0.08)


@pytest.mark.parametrize("model,modes,interval,shipped", V.MODELS)
def test_resident_valid_steps_is_valid_steps(tmp_path, model, modes, interval, shipped):
    val, files = V.write_val_dir(tmp_path / "bench")
    net = _net(tmp_path, model, modes, interval, shipped)
    net.train()
    host_opt, res_opt = _opt(val, tmp_path / "host"), _opt(val, tmp_path / "resident")
    vset = finetune_lut.DeviceValSet(res_opt, workers=2)
    assert [s["name"] for s in vset.sets] == ["Set5", "Set14"] and len(vset.shapes) == 5
    seen = []
    for it in (7, 9):
        a_lines, b_lines = [], []
        a = finetune_lut.valid_steps(net, host_opt, it, a_lines.append)
        b = finetune_lut.resident_valid_steps(net, vset, res_opt, it, b_lines.append)
        assert net.training
        vset.join()
        assert a_lines == b_lines and len(a_lines) == 2 and a == b
        _same_results(host_opt.valResults, res_opt.valResults)
        seen.append((a, _same_files(str(tmp_path / "host"), str(tmp_path / "resident"), files)))
        _perturb(net)                                   # the second point: both paths move together, the files are overwritten
    assert seen[0][0] != seen[1][0]
    assert all(not np.array_equal(seen[0][1][k], seen[1][1][k]) for k in seen[0][1])
    vset.close()


@pytest.mark.parametrize("model,modes,interval,shipped", V.MODELS)
def test_resident_engine_valid_steps_is_engine_valid_steps(tmp_path, model, modes, interval, shipped):
    from mulut_amd.engine import MuLUTEngine
    val, files = V.write_val_dir(tmp_path / "bench")
    net = _net(tmp_path, model, modes, interval, shipped)
    opt = _opt(val, tmp_path / "out")
    vset = finetune_lut.DeviceValSet(opt, workers=2)
    engine = MuLUTEngine(0).configure(2, modes, 4, interval)
    seen = []
    for it in (7, 9):
        a_lines, b_lines = [], []
        a = finetune_lut.engine_valid_steps(net, engine, opt, it, a_lines.append)
        b = finetune_lut.resident_engine_valid_steps(net, engine, vset, opt, it, b_lines.append)
        assert a_lines == b_lines and len(a_lines) == 2
        _same_results(a, b)
        seen.append(a)
        _perturb(net)
    assert any(bits(seen[0][ds]).tolist() != bits(seen[1][ds]).tolist() for ds in seen[0])
    engine.close()
    vset.close()


# ------------------------------------------------------------------------------------------------------------------- the driver
def _drive(tmp_path, capsys, name, val, extra):
    exp = V.write_exp(tmp_path / name, "sdy", 4, True)
    finetune_lut.main(["--stages", "2", "--modes", "sdy", "-e", exp, "--trainDir", os.path.join(GOLDEN, "Set5"), "--batchSize", "4",
                       "--cropSize", "12", "--totalIter", "4", "--displayStep", "2", "--valStep", "2", "--seed", "5", "--valDir", val,
                       "--valEngine"] + extra)
    lines = capsys.readouterr().out.splitlines()
    lines = [re.sub(r"rT:[0-9.eE+-]+", "rT:*", ln).replace(exp, "EXP") for ln in lines]
    tables = {fn: np.load(os.path.join(exp, fn)) for fn in sorted(os.listdir(exp)) if fn.startswith("LUT_ft_")}
    return exp, lines, tables


def test_driver_with_and_without_the_resident_validation(tmp_path, capsys):
    """finetune_lut.main, 4 iterations, validation at 1, 2 and 4, --valEngine: the log (apart from rT) and the exported tables do not
    depend on --valResident; --valSave every leaves the last point's bytes on disk after finish(), last the same files, never none;
    a memory limit of 1 byte falls back to valid_steps with one log line and the same results."""
    val, files = V.write_val_dir(tmp_path / "bench")
    host_exp, host_lines, host_tables = _drive(tmp_path, capsys, "host", val, [])
    assert len(host_tables) == 6 and sum("AVG PSNR" in ln for ln in host_lines) == 6 and sum("AVG LUT PSNR" in ln for ln in host_lines) == 6
    assert any("rT:*" in ln for ln in host_lines)
    for save in ("every", "last", "never"):
        exp, lines, tables = _drive(tmp_path, capsys, "resident_" + save, val, ["--valResident", "--valSave", save, "--valWorkers", "2"])
        assert lines == host_lines, save
        assert list(tables) == list(host_tables) and all(np.array_equal(tables[k], host_tables[k]) for k in tables)
        if save == "never":
            assert not os.path.isdir(os.path.join(exp, "val")) or not any(fs for _, _, fs in os.walk(os.path.join(exp, "val")))
        else:
            _same_files(os.path.join(host_exp, "val"), os.path.join(exp, "val"), files)
    exp, lines, tables = _drive(tmp_path, capsys, "fallback", val, ["--valResident", "--valMaxBytes", "1"])
    fell = [ln for ln in lines if "validation runs on the host loop" in ln]
    assert len(fell) == 1 and [ln for ln in lines if ln not in fell] == host_lines
    assert all(np.array_equal(tables[k], host_tables[k]) for k in tables)
    _same_files(os.path.join(host_exp, "val"), os.path.join(exp, "val"), files)
