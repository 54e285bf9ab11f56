"""What a context holds of its tables, read back (-m gpu): mulut_read_table_image of include/mulut.h / MuLUTEngine.read_table_image,
and what is built on installing a module's current tables into an engine: MuLUT.install_into, finetune_lut --valEngine and
transfer(..., engine=).

Bars: the three device images of a table equal, byte for byte and in size, a NumPy restatement of their documented formats
(tests/tables_cases.py); outputs equal the reference (oracle.c_oracle) for the tables the module would export; the driver's engine
score equals what mulut_amd.test_lut computes from the exported files."""
import functools
import os

import numpy as np
import pytest
from PIL import Image

import abi_sequences as A
import tables_cases as T
from conftest import GOLDEN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine  # noqa: E402
from mulut_amd.synth import natural_frames  # noqa: E402


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def check_images(e, stage, mode, iv, u, table, what):
    for which, want in enumerate(T.images(iv, u, mode, table)):
        got = e.read_table_image(stage, mode, which)
        assert len(got) == len(want), (what, which, len(got), len(want))
        if got != want:
            d = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
            raise AssertionError("%s: image %d differs in %d of %d bytes, first at %s" % (what, which, d.size, len(got), d[:8]))


# ------------------------------------------------------------------------------------------------------------------------ images
@pytest.mark.parametrize("iv,u,mode", T.SHAPES, ids=lambda v: str(v))
def test_images_are_what_the_formats_say(iv, u, mode):
    """every row size at interval 4 with a band pattern and a wide one, intervals 5 and 6: into an empty slot, then rewritten in
    place over what the round before left (random rows, all -128, all 127, a ramp)"""
    e = MuLUTEngine(0).configure(1, mode, u, iv)
    assert [e.read_table_image(1, mode, w) for w in range(3)] == [b"", b"", b""]
    for kind in T.KINDS:
        t = T.table(kind, iv, u)
        e.set_lut(1, mode, t)
        check_images(e, 1, mode, iv, u, t, kind)
    band = iv == 4 and mode in "sdy"
    sizes = [len(e.read_table_image(1, mode, w)) for w in range(3)]
    assert (sizes[1] > 0) == band and (sizes[2] > 0) == (band and u == 4), sizes
    e.close()


def test_images_follow_a_table_of_another_shape_and_a_side_stream():
    e = MuLUTEngine(0)
    for u in (4, 1, 2, 4):
        t = T.table("random", 4, u, seed=u)
        e.set_lut(2, "d", t)
        with torch.cuda.stream(torch.cuda.Stream()):
            check_images(e, 2, "d", 4, u, t, "v_num %d" % (u * u))
    assert e.read_table_image(3, "d", 0) == b""
    with pytest.raises(ValueError):
        e.read_table_image(2, "q", 0)
    for stage, which in ((0, 0), (9, 0), (2, 3), (2, -1)):
        with pytest.raises(Exception, match="-1"):
            e.read_table_image(stage, "d", which)
    e.close()


# ------------------------------------------------------------------------------------------------------------------ install_into
@functools.lru_cache(maxsize=None)
def frames():
    """2 x 70 x 67 x 3: a 3-pixel tile column, H % 4 == 2, more than one wave tile per wave; a photograph-like frame and noise"""
    img = np.empty((2, 70, 67, 3), np.uint8)
    img[0] = natural_frames(1, 270, 267, 3, seed=11)[0, 100:170, 100:167]
    img[1] = np.random.default_rng(11).integers(0, 256, (70, 67, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


def write_luts(folder, tables, scale, interval, name="LUT"):
    for (s, m), t in tables.items():
        np.save(os.path.join(str(folder), "%s_x%d_%dbit_int8_s%d_%s.npy" % (name, scale, interval, s, m)), t)


@pytest.mark.parametrize("stages,modes,scale,interval", [(2, "sdy", 4, 4), (3, "sdy", 2, 4), (2, "sdy", 4, 5), (2, "se", 3, 4)])
def test_install_into_leaves_the_engine_with_the_exported_tables(tmp_path, stages, modes, scale, interval):
    """the module's parameters, moved off the int8 grid (beyond +-1 too), installed twice: the engine's images are those of the
    tables export_int8() gives -- NumPy's round(clip(w, -1, 1) * 127) -- and its outputs the reference's for them"""
    from mulut_amd.finetune import MuLUTWide
    rng = np.random.default_rng(stages + scale + interval)
    tables = {(s, m): A.make_table(rng, interval, scale * scale if s == stages else 1, True) for s in range(1, stages + 1) for m in modes}
    write_luts(tmp_path, tables, scale, interval)
    net = MuLUTWide(str(tmp_path), stages, list(modes), upscale=scale, interval=interval).cuda()
    e = MuLUTEngine(0).configure(stages, modes, scale, interval)
    with pytest.raises(ValueError):
        net.install_into(MuLUTEngine(0).configure(stages, modes, scale % 4 + 1, interval))
    with pytest.raises(ValueError):
        net.install_into(MuLUTEngine(0).configure(stages, modes[::-1], scale, interval))
    x = dev(frames()[:, :40, :37] if "e" in modes else frames())
    for rnd in range(2):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(dev((rng.standard_normal(tuple(p.shape)) * 0.05).astype(np.float32)))
        assert net.install_into(e) is e
        now = {(int(k[8]), k[10]): T.np_export(p.detach().cpu().numpy()) for k, p in net.named_parameters()}      # weight_s{stage}_{mode}
        assert sorted(now) == sorted(tables) and all(not np.array_equal(now[k], tables[k]) for k in tables)
        for (s, m), t in now.items():
            check_images(e, s, m, interval, scale if s == stages else 1, t, "round %d s%d_%s" % (rnd, s, m))
        want = np.stack([A.ref_pipeline(now, stages, modes, scale, im, interval) for im in x.cpu().numpy()])
        got = e.pipeline(x).cpu().numpy()
        assert np.array_equal(got, want), (rnd, int((got != want).sum()))
        tables = now
    e.close()


# ------------------------------------------------------------------------------------------------------------------------ driver
def test_driver_scores_the_deployed_path(tmp_path, capsys):
    """finetune_lut --valEngine on two synthetic pairs (LR 24 x 20): the last engine line of the log carries what
    mulut_amd.test_lut prints for the exported LUT_ft files, the per-image doubles are equal, and without the flag no such line."""
    from mulut_amd import finetune_lut, test_lut
    root = tmp_path / "bench" / "Set5"
    os.makedirs(root / "HR")
    os.makedirs(root / "LR_bicubic" / "X4")
    hr = natural_frames(2, 96, 80, 3, seed=21)
    for n in range(2):
        Image.fromarray(hr[n]).save(root / "HR" / ("im%d.png" % n))
        lr = hr[n].reshape(24, 4, 20, 4, 3).mean(axis=(1, 3)).round().astype(np.uint8)
        Image.fromarray(lr).save(root / "LR_bicubic" / "X4" / ("im%d.png" % n))
    exp = tmp_path / "exp"
    exp.mkdir()
    for s in (1, 2):
        for m in "sdy":
            t = np.load(os.path.join(GOLDEN, "luts", "LUT_ft_x4_4bit_int8_s%d_%s.npy" % (s, m)))
            np.save(exp / ("LUT_x4_4bit_int8_s%d_%s.npy" % (s, m)), t)
    args = ["--stages", "2", "--modes", "sdy", "-e", str(exp), "--trainDir", str(root), "--valDir", str(tmp_path / "bench"),
            "--batchSize", "4", "--cropSize", "16", "--totalIter", "4", "--valStep", "2", "--displayStep", "2", "--seed", "0", "--lr0", "1e-3"]
    plain = []
    finetune_lut.finetune(finetune_lut.build_parser().parse_args(args), log=plain.append)
    assert plain and not any("LUT PSNR" in line for line in plain)
    log = []
    opt = finetune_lut.build_parser().parse_args(args + ["--valEngine"])
    finetune_lut.finetune(opt, log=log.append)
    # (the rest of the log keeps its lines: what they print of the training run is not bit-reproducible, its gradients are atomic sums)
    assert [line.split(":")[0] for line in log if "LUT PSNR" not in line] == [line.split(":")[0] for line in plain]
    assert len([line for line in log if "AVG PSNR" in line]) == len([line for line in plain if "AVG PSNR" in line]) == 3
    engine_lines = [line for line in log if "LUT PSNR" in line]
    assert [line.split(" | ")[0] for line in engine_lines] == ["Iter 1", "Iter 2", "Iter 4"], engine_lines
    capsys.readouterr()
    res = test_lut.main(["--stages", "2", "--modes", "sdy", "-e", str(exp), "--testDir", str(tmp_path / "bench"),
                         "--resultRoot", str(tmp_path / "results"), "--deviceMetrics"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("Dataset Set5 | AVG LUT PSNR: ")
    assert engine_lines[-1] == "Iter 4 | " + line
    assert np.array_equal(np.asarray(opt.valEngineResults["Set5"]), np.asarray(res["Set5"]))
    assert res["Set5"].shape == (2, 2)


# ---------------------------------------------------------------------------------------------------------------------- transfer
def test_transfer_leaves_the_engine_with_the_returned_tables():
    from types import SimpleNamespace
    from mulut_amd import network, transfer_to_lut
    torch.manual_seed(0)
    net = network.SRNets(nf=8, scale=2, modes=list("sdy"), stages=1).cuda()
    opt = SimpleNamespace(stages=1, modes="sdy", scale=2, interval=4, expDir="")
    e = MuLUTEngine(0).configure(1, "sdy", 2, 4)
    tabs = transfer_to_lut.transfer(net, opt, device=torch.device("cuda"), save=False, engine=e)
    plain = transfer_to_lut.transfer(net, opt, device=torch.device("cuda"), save=False)
    for m in "sdy":
        key = "s1_" + m
        assert tabs[key].shape == (83521, 1, 2, 2) and tabs[key].dtype == np.int8 and np.array_equal(tabs[key], plain[key])
        check_images(e, 1, m, 4, 2, tabs[key].reshape(83521, 4), key)
    x = dev(frames())
    want = np.stack([A.ref_pipeline({(1, m): tabs["s1_" + m].reshape(83521, 4) for m in "sdy"}, 1, "sdy", 2, im, 4) for im in frames()])
    assert np.array_equal(e.pipeline(x).cpu().numpy(), want)
    e.close()
