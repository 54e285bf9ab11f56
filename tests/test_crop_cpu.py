"""The device-resident training set without a GPU: DeviceCropProvider's host half (the scan, the packed pool, the pair table and the
order in which the draws consume random.Random(seed)) against CropProvider, and mulut_ft_crop_batch's host half (refusals, launch
configuration) as a stand-alone program under AddressSanitizer / UndefinedBehaviorSanitizer against tests/host_emul/fake_hip.cpp."""
import os
import sys

import numpy as np
import pytest
import torch

import crop_cases as CC
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return {s: CC.write_set(tmp_path_factory.mktemp("crops_x%d" % s), s) for s in (2, 3, 4)}


@pytest.fixture
def cuda_is_identity(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)


@pytest.mark.parametrize("sz", [1, 5, 48])
@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("seed", [0, 1, 20240229])
def test_draws_consume_the_rng_in_the_host_providers_order(sets, cuda_is_identity, seed, scale, sz):
    """4 consecutive batches: the draws of DeviceCropProvider's host half, applied with np.fliplr / flipud / rot90, are
    CropProvider.next() bit for bit."""
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider
    B = 6
    host = CropProvider(sets[scale], scale, sz, B, seed)
    dev = DeviceCropProvider(sets[scale], scale, sz, B, seed)
    for _ in range(4):
        draws = dev.draw()
        assert draws.dtype == np.int32 and draws.shape == (B, 6)
        im, lb = CC.apply_draws(host.pairs, draws, sz, scale)
        want_im, want_lb = host.next()
        assert im.shape == (B, 1, sz, sz) and lb.shape == (B, 1, sz * scale, sz * scale)
        assert np.array_equal(im, want_im.numpy()) and np.array_equal(lb, want_lb.numpy())


@pytest.mark.parametrize("scale,sz", [(2, 5), (4, 57), (3, 58)])
def test_pool_and_pair_table_hold_the_host_providers_pairs_in_order(sets, cuda_is_identity, scale, sz):
    """The packed bytes and the 40-byte entries of the table are the arrays CropProvider holds, in its order -- also when the patch
    size makes it drop a pair (sz 58: a_rgb and c_tight have 57 rows)."""
    from mulut_amd.finetune_lut import CropProvider, DeviceCropProvider, TrainingSetTooLarge
    host = CropProvider(sets[scale], scale, sz, 2, 0)
    dev = DeviceCropProvider(sets[scale], scale, sz, 2, 0)
    assert len(host.pairs) == (3 if sz == 58 else 5)
    table = dev.table.numpy()
    assert table.dtype == np.int32 and table.shape == (len(host.pairs), 10)
    pool, end = dev.pool.numpy(), 0
    for row, (lr, hr) in zip(table, host.pairs):
        lr_off, hr_off = (int(v) for v in row[:4].view(np.int64))
        assert (lr_off, hr_off) == (end, end + lr.size)
        assert row[4:].tolist() == [lr.shape[0], lr.shape[1], hr.shape[0], hr.shape[1], lr.shape[2], 0]
        assert np.array_equal(pool[lr_off:lr_off + lr.size].reshape(lr.shape), lr)
        assert np.array_equal(pool[hr_off:hr_off + hr.size].reshape(hr.shape), hr)
        end = hr_off + hr.size
    assert end == dev.pool_bytes == pool.size
    # a set over the caller's limit is refused before anything is uploaded, and hands over the loaded host provider
    with pytest.raises(TrainingSetTooLarge) as e:
        DeviceCropProvider(sets[scale], scale, sz, 2, 7, max_bytes=end - 1)
    assert (e.value.nbytes, e.value.limit) == (end, end - 1) and isinstance(e.value.host, CropProvider)
    want = CropProvider(sets[scale], scale, sz, 2, 7).next()
    got = e.value.host.next()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert DeviceCropProvider(sets[scale], scale, sz, 2, 7, max_bytes=end).pool_bytes == end


def test_driver_takes_the_host_provider_on_request(tmp_path):
    from mulut_amd import finetune_lut
    opt = finetune_lut.build_parser().parse_args(["-e", str(tmp_path)])
    assert opt.hostData is False
    assert finetune_lut.build_parser().parse_args(["-e", str(tmp_path), "--hostData"]).hostData is True


def test_host_half_refusals_and_launch_configuration_under_sanitizers(tmp_path):
    """mulut_ft_data.hip's host half + fake_hip.cpp + crop_host.cpp (its own main), -fsanitize=address,undefined, run as a program."""
    from mulut_amd import _native
    import host_abi as tool
    if _native._hipcc() is None:
        pytest.skip("no hipcc")
    assert "mulut_ft_data.hip" in _native.SOURCES and "mulut_ft_crop_batch" in _native.EXPORTS
    r = tool.run(tool.build(str(tmp_path), tool.CSRC, "crop_host", ["mulut_ft_data.hip"]))
    print(r.stdout)
    assert r.stderr == "", r.stderr[-4000:]
    assert r.returncode == 0 and "UNEXPECTED" not in r.stdout and r.stdout.endswith("\n0 unexpected\n")
    lines = r.stdout.splitlines()
    assert "B 1 sz 1 x1 -> 0 [launch ft_crop_kernel grid 1,1,1 block 256,1,1 lds 0]" in lines
    assert "B 256 sz 48 x4 -> 0 [launch ft_crop_kernel grid 1280,1,1 block 256,1,1 lds 0]" in lines
    assert sum(" -> -1 []" in ln for ln in lines) == 14 and sum(" -> -5 []" in ln for ln in lines) == 7 and "device 3 -> -7 []" in lines
