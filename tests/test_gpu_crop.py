"""mulut_ft_crop_batch and DeviceCropProvider on the GPU: the batches are CropProvider's (sr/data.py:91-121) bit for bit, for every
transform, channel and window position, past 2^32 bytes of pool, on a side stream, with the host running ahead; draws the kernel must
refuse come out as zeros and are counted; the driver trains with either provider."""
import ctypes
import os

import numpy as np
import pytest
import torch

import crop_cases as CC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from mulut_amd import _native
    return _native.load()


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return {s: CC.write_set(tmp_path_factory.mktemp("crops_x%d" % s), s) for s in (2, 3, 4)}


def crop(lib, pool, pool_bytes, table, draws, sz, scale, count_bad=True, stream=None, fill=None):
    """One mulut_ft_crop_batch call on torch tensors -> (im, lb, bad or None); `fill`: what the outputs hold before the call."""
    draws = torch.tensor(np.asarray(draws, np.int32).reshape(-1, 6), device="cuda")
    B = draws.shape[0]
    im = torch.empty((B, 1, sz, sz), dtype=torch.float32, device="cuda")
    lb = torch.empty((B, 1, sz * scale, sz * scale), dtype=torch.float32, device="cuda")
    if fill is not None:
        im.fill_(fill)
        lb.fill_(fill)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda") if count_bad else None
    torch.cuda.synchronize()      # (inputs made on the current stream; the call may go to another one)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = lib.mulut_ft_crop_batch(0, pool.data_ptr(), pool_bytes, table.data_ptr(), table.shape[0], draws.data_ptr(), B, sz, scale,
                                 im.data_ptr(), lb.data_ptr(), bad.data_ptr() if count_bad else None, st)
    assert rc == 0, lib.mulut_strerror(rc)
    (stream or torch.cuda.current_stream()).synchronize()
    return im, lb, bad


def same_batches(dev, host, n):
    got = [dev.next() for _ in range(n)]      # (all queued before the first comparison waits for the device)
    for k, (im, lb) in enumerate(got):
        want_im, want_lb = host.next()
        assert im.shape == want_im.shape and lb.shape == want_lb.shape and im.dtype == lb.dtype == torch.float32
        assert torch.equal(im, want_im), "im of batch %d" % k
        assert torch.equal(lb, want_lb), "lb of batch %d" % k
    assert int(dev.bad.item()) == 0


def test_parity_with_the_host_provider_on_set5():
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider
    path = os.path.join(GOLDEN, "Set5")
    same_batches(DeviceCropProvider(path, 4, 48, 8, seed=3), CropProvider(path, 4, 48, 8, seed=3), 4)


@pytest.mark.parametrize("sz", [1, 5, 48, 57])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_parity_with_the_host_provider_on_the_synthetic_set(sets, scale, sz):
    """sz 57: no multiple of 4 (float stores), the last row and column of a_rgb and c_tight, two tiles per LR side; sz 1 and 5: one
    partial tile; scale 3 x sz 5: an lb plane that is no multiple of 4 either."""
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider
    same_batches(DeviceCropProvider(sets[scale], scale, sz, 8, seed=sz * 10 + scale), CropProvider(sets[scale], scale, sz, 8, seed=sz * 10 + scale), 4)


@pytest.mark.parametrize("scale,sz", [(3, 5), (4, 48), (2, 34)])
def test_every_transform_channel_and_corner(lib, sets, scale, sz):
    """An explicit draw table: every (flips, k) x channel x window corner (i and j at 0 and at their maxima) of an RGB pair, the grey
    pair and the pair whose HR is wider than scale * LR, against np.fliplr / flipud / rot90.  (3, 5): float stores on both planes;
    (4, 48): 16-byte stores, 2 x 2 and 6 x 6 tiles with partial ones; (2, 34): 16-byte stores on lb only, a 2-pixel last tile."""
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider
    dev, pairs = DeviceCropProvider(sets[scale], scale, sz, 1), CropProvider(sets[scale], scale, sz, 1).pairs
    draws = []
    for n in (0, 1, 3):
        h, w, ch = pairs[n][0].shape
        for c in range(ch):
            for i in (0, h - sz):
                for j in (0, w - sz):
                    draws += [(n, i, j, c, flips, k) for flips in range(4) for k in range(4)]
    assert len(draws) == 7 * 4 * 16
    im, lb, bad = crop(lib, dev.pool, dev.pool_bytes, dev.table, draws, sz, scale, fill=7.0)
    want_im, want_lb = CC.apply_draws(pairs, draws, sz, scale)
    assert int(bad.item()) == 0
    wrong = [d for d, a, b, x, y in zip(draws, im.cpu().numpy(), want_im, lb.cpu().numpy(), want_lb) if not (np.array_equal(a, b) and np.array_equal(x, y))]
    assert not wrong, "%d of %d samples differ, first %r" % (len(wrong), len(draws), wrong[:4])


def test_all_256_byte_values_convert_as_numpy_does(lib, sets):
    """The e_bytes pair holds every byte value in each channel: the whole 64 x 64 LR image and its HR, untransformed."""
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider
    dev, pairs = DeviceCropProvider(sets[2], 2, 64, 1), CropProvider(sets[2], 2, 64, 1).pairs
    assert len(pairs) == 1 and all(len(np.unique(pairs[0][0][:, :, c])) == 256 for c in range(3))
    draws = [(0, 0, 0, c, 0, 0) for c in range(3)]
    im, lb, _ = crop(lib, dev.pool, dev.pool_bytes, dev.table, draws, 64, 2)
    want_im, want_lb = CC.apply_draws(pairs, draws, 64, 2)
    assert len(np.unique(want_im)) == 256
    assert np.array_equal(im.cpu().numpy(), want_im) and np.array_equal(lb.cpu().numpy(), want_lb)


def test_host_running_ahead_never_rewrites_a_draw_buffer_in_flight(sets):
    """64 next() calls with nothing waiting in between -- twice round the ring of pinned buffers -- then every batch against the host
    provider: a slot rewritten while its copy was still queued would show as another batch's samples."""
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider
    dev = DeviceCropProvider(sets[4], 4, 48, 8, seed=11)
    assert 64 >= 2 * dev.RING
    same_batches(dev, CropProvider(sets[4], 4, 48, 8, seed=11), 64)


def test_offsets_past_4_gib(lib):
    """A pool of 2^32 + 64 KiB bytes (only the allocation is large) with one tiny pair at offset 2^32 + 1."""
    rng = np.random.default_rng(5)
    lr, hr = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8), rng.integers(0, 256, (12, 14, 3), dtype=np.uint8)
    nbytes, off = (1 << 32) + (64 << 10), (1 << 32) + 1
    pool = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    pool[off - 4096:off + 8192] = 0
    pool[:8192] = 0      # (where offsets cut to 32 bits would read)
    pool[off:off + lr.size] = torch.from_numpy(lr.reshape(-1)).cuda()
    pool[off + lr.size:off + lr.size + hr.size] = torch.from_numpy(hr.reshape(-1)).cuda()
    table = np.zeros((1, 10), np.int32)
    table.view(np.int64)[0, :2] = off, off + lr.size
    table[0, 4:9] = 6, 7, 12, 14, 3
    draws = [(0, i, j, c, flips, k) for (i, j) in ((0, 0), (1, 2)) for c in range(3) for flips in (0, 3) for k in range(4)]
    im, lb, bad = crop(lib, pool, nbytes, torch.from_numpy(table).cuda(), draws, 5, 2)
    want_im, want_lb = CC.apply_draws([(lr, hr)], draws, 5, 2)
    assert int(bad.item()) == 0 and want_im.any()
    assert np.array_equal(im.cpu().numpy(), want_im) and np.array_equal(lb.cpu().numpy(), want_lb)


@pytest.mark.parametrize("scale,sz", [(4, 48), (3, 5)])
def test_draws_the_kernel_must_refuse_are_zeroed_and_counted(lib, sets, scale, sz):
    """pool_bytes is SMALLER than the tensor: whatever a broken guard read past it would be owned, non-zero memory.  Outputs are
    pre-filled, so a refused sample must have been written as zeros; the legal samples between the refused ones are intact."""
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider
    dev, pairs = DeviceCropProvider(sets[scale], scale, sz, 1), CropProvider(sets[scale], scale, sz, 1).pairs
    P, n = dev.pool_bytes, len(pairs)
    pool = torch.full((P + pairs[0][1].size + 64,), 200, dtype=torch.uint8, device="cuda")
    pool[:P] = dev.pool
    t = dev.table.cpu().numpy()
    extra = np.repeat(t[:1], 5, axis=0)      # five more entries, all copies of pair 0 (a_rgb, LR 57 x 86) with one field changed
    extra[0].view(np.int64)[1] = P                                   # n:     hr_off at pool_bytes (its bytes lie in the tensor's tail)
    extra[1].view(np.int64)[1] = P - 10                              # n + 1: the HR image straddles pool_bytes
    extra[2].view(np.int64)[0] = -1                                  # n + 2: a negative offset
    extra[3][6] -= 1                                                 # n + 3: hr_h one short of scale * lr_h: the last LR row has no HR window
    extra[4][8] = 0                                                  # n + 4: no channels
    table = torch.from_numpy(np.concatenate([t, extra])).cuda()
    h, w, ch = pairs[0][0].shape
    gh, gw, _ = pairs[1][0].shape
    good = [(0, h - sz, w - sz, 2, 1, 1), (1, gh - sz, 0, 0, 2, 3), (n + 3, h - sz - 1, 3, 1, 3, 2), (3, 0, 1, 0, 0, 1)]
    refused = [(-1, 0, 0, 0, 0, 0), (n + 5, 0, 0, 0, 0, 0), (0, 0, 0, ch, 0, 0), (1, 0, 0, 1, 0, 0), (0, 0, 0, -1, 0, 0),
               (0, h - sz + 1, 0, 0, 0, 0), (0, 0, w - sz + 1, 0, 0, 0), (0, -1, 0, 0, 0, 0), (0, 0, -1, 0, 0, 0),
               (0, 2 ** 31 - 1, 0, 0, 0, 0), (n, 0, 0, 0, 0, 0), (n + 1, 0, 0, 0, 0, 0), (n + 2, 0, 0, 0, 0, 0),
               (n + 3, h - sz, 0, 0, 0, 0), (n + 4, 0, 0, 0, 0, 0)]
    draws, is_good = [], []
    for k, r in enumerate(refused):      # good, refused, good, refused, ... and two refused samples side by side at the end
        draws += [good[k % len(good)], r]
        is_good += [True, False]
    draws.append(refused[0])
    is_good.append(False)
    im, lb, bad = crop(lib, pool, P, table, draws, sz, scale, fill=7.0)
    all_pairs = pairs + [pairs[0]] * 5
    ok_draws = [d for d, g in zip(draws, is_good) if g]
    want_im, want_lb = CC.apply_draws(all_pairs, ok_draws, sz, scale)
    g = torch.tensor(is_good)
    assert int(bad.item()) == len(refused) + 1
    assert not im[~g].any() and not lb[~g].any()
    assert np.array_equal(im[g].cpu().numpy(), want_im) and np.array_equal(lb[g].cpu().numpy(), want_lb)


def test_side_stream_and_no_bad_counter(lib, sets):
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider
    dev, host = DeviceCropProvider(sets[3], 3, 48, 8, seed=2), CropProvider(sets[3], 3, 48, 8, seed=2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = [dev.next() for _ in range(2)]
    side.synchronize()
    for im, lb in got:
        want_im, want_lb = host.next()
        assert torch.equal(im, want_im) and torch.equal(lb, want_lb)
    draws = [(0, 1, 2, 1, 3, 1), (9, 0, 0, 0, 0, 0), (1, 3, 0, 0, 1, 2)]      # the middle one is refused, and nobody counts
    im, lb, bad = crop(lib, dev.pool, dev.pool_bytes, dev.table, draws, 48, 3, count_bad=False, stream=side, fill=7.0)
    want_im, want_lb = CC.apply_draws(host.pairs, [draws[0], draws[2]], 48, 3)
    assert bad is None and not im[1].any() and not lb[1].any()
    assert np.array_equal(im[[0, 2]].cpu().numpy(), want_im) and np.array_equal(lb[[0, 2]].cpu().numpy(), want_lb)


def _experiment(tmp_path, name):
    exp = tmp_path / name
    exp.mkdir()
    for s in (1, 2):
        for m in "sdy":
            t = np.load(os.path.join(GOLDEN, "luts", "LUT_ft_x4_4bit_int8_s%d_%s.npy" % (s, m)))
            rng = np.random.default_rng(s * 7 + ord(m))      # a perturbed copy, so that there is something to learn
            np.save(exp / ("LUT_x4_4bit_int8_s%d_%s.npy" % (s, m)), np.clip(t.astype(np.int32) + rng.integers(-12, 13, t.shape), -127, 127).astype(np.int8))
    return exp


@pytest.mark.parametrize("host_data", [False, True])
def test_driver_trains_with_either_provider(tmp_path, monkeypatch, host_data):
    """60 iterations on the Set5 pairs with --seed: the loss falls, the LUT_ft_* files appear under the reference's names in int8, one
    loss per iteration comes back and the log keeps its line.  (Losses of two runs are not compared: the backward's atomics reorder sums.)"""
    from mulut_amd import finetune_lut
    made = []

    def recording(cls):
        real = getattr(finetune_lut, cls)

        class Recorded(real):
            def __init__(self, *a, **k):
                made.append(cls)
                real.__init__(self, *a, **k)
        return Recorded

    for cls in ("CropProvider", "DeviceCropProvider"):
        monkeypatch.setattr(finetune_lut, cls, recording(cls))
    exp, lines = _experiment(tmp_path, "exp"), []
    opt = finetune_lut.build_parser().parse_args(["--stages", "2", "--modes", "sdy", "-e", str(exp), "--trainDir", os.path.join(GOLDEN, "Set5"),
                                                  "--batchSize", "16", "--cropSize", "24", "--totalIter", "60", "--displayStep", "25", "--lr0", "1e-3",
                                                  "--seed", "0", "--valStep", "0"] + (["--hostData"] if host_data else []))
    losses = finetune_lut.finetune(opt, log=lines.append)
    assert made == (["CropProvider"] if host_data else ["DeviceCropProvider"])      # (the device provider scans for itself: ft_data.scan_pairs)
    assert len(losses) == 60 and all(isinstance(v, float) and np.isfinite(v) for v in losses)
    assert np.mean(losses[-15:]) < np.mean(losses[:15])
    shown = [ln for ln in lines if "Iter:" in ln]
    assert len(shown) == 2 and shown[0].startswith("%s | Iter:    25, Sample:   400, GPixel:%.2e, rT:" % (exp, sum(losses[:25]) / 25))
    assert float(shown[1].split("rT:")[1]) > 0
    for s in (1, 2):
        for m in "sdy":
            t = np.load(exp / ("LUT_ft_x4_4bit_int8_s%d_%s.npy" % (s, m)))
            assert t.dtype == np.int8 and t.shape == (83521, 16 if s == 2 else 1)


def test_driver_falls_back_to_the_host_provider_when_the_set_does_not_fit(tmp_path, monkeypatch):
    from mulut_amd import finetune_lut
    exp, lines = _experiment(tmp_path, "exp"), []
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (1000, 1 << 30))
    took = []
    real_next = finetune_lut.CropProvider.next
    monkeypatch.setattr(finetune_lut.CropProvider, "next", lambda self: (took.append(1), real_next(self))[1])
    losses = finetune_lut.main(["--stages", "2", "--modes", "sdy", "-e", str(exp), "--trainDir", os.path.join(GOLDEN, "Set5"), "--batchSize", "4",
                                "--cropSize", "24", "--totalIter", "3", "--displayStep", "2", "--seed", "0", "--valStep", "0"])
    assert len(losses) == 3 and len(took) == 3
