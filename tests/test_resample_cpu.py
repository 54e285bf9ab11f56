"""Pillow's bicubic resize without a GPU: the NumPy restatement of tests/resample_cases.py against Pillow itself, the library's
coefficient tables (mulut_resample_coeffs, host only) against the restatement, every refusal of the mulut_resample_* entry points
through the loaded library, and their host half as a stand-alone program under AddressSanitizer / UndefinedBehaviorSanitizer against
tests/host_emul/fake_hip.cpp."""
import ctypes
import os
import sys

import numpy as np
import pytest

import resample_cases as RC
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_restatement_equals_pillow_on_the_case_list():
    cases = RC.cases()
    assert len(cases) >= 300 and {c[3] for c in cases} == {0, 3}
    for h, w, kind, ch, oh, ow in cases:
        a = RC.image(h, w, kind, ch)
        got, want = RC.resize(a, oh, ow), RC.pil_resize(a, oh, ow)
        assert got.shape == want.shape and np.array_equal(got, want), (h, w, kind, ch, oh, ow)


def _axes():
    for n in range(1, 601):
        for s in RC.SCALES:
            if n // s:
                yield n, n // s
            yield n, n * s
    yield from RC.PAIRS


def test_library_coefficients_equal_the_restatement():
    from mulut_amd import resample
    count = 0
    for insz, outsz in _axes():
        kk, xmin, n = resample.coeffs(insz, outsz)
        wkk, wxmin, wn = RC.coeffs(insz, outsz)
        assert kk.shape == wkk.shape and np.array_equal(kk, wkk), (insz, outsz)
        assert np.array_equal(xmin, wxmin) and np.array_equal(n, wn), (insz, outsz)
        assert xmin.min() >= 0 and (xmin + n).max() <= insz and n.min() >= 1
        count += 1
    assert count > 3000


def test_refusals_come_before_a_pointer_is_followed():
    """Through the loaded library, without a device: every pointer handed over is an address nothing may follow."""
    from mulut_amd import _native
    lib = _native.load()
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -5, -9
    i32p = ctypes.POINTER(ctypes.c_int32)
    bad = ctypes.cast(0x1000, i32p)
    null = ctypes.cast(None, i32p)
    assert lib.mulut_resample_coeffs(8, 2, null, bad, bad, 64) == EINVAL
    assert lib.mulut_resample_coeffs(8, 2, bad, null, bad, 64) == EINVAL
    assert lib.mulut_resample_coeffs(8, 2, bad, bad, null, 64) == EINVAL
    for v in (0, -1):
        assert lib.mulut_resample_coeffs(v, 2, bad, bad, bad, 64) == EINVAL
        assert lib.mulut_resample_coeffs(8, v, bad, bad, bad, 64) == EINVAL
    assert lib.mulut_resample_coeffs(2 ** 31 - 1, 1, bad, bad, bad, 64) == EUNSUPPORTED
    assert lib.mulut_resample_coeffs(8, 2, bad, bad, bad, 33) == EWORKSPACE
    plan = ctypes.c_void_p(0x1000)
    assert lib.mulut_resample_plan_create(0, 8, 8, 2, 2, None) == EINVAL
    for k in range(4):
        for v in (0, -1):
            dims = [8, 8, 2, 2]
            dims[k] = v
            plan.value = 0x1000
            assert lib.mulut_resample_plan_create(0, *dims, ctypes.byref(plan)) == EINVAL and not plan.value
    for dims in ((1 << 16, 1 << 15, 2, 2), (2, 2, 1 << 15, 1 << 16), (1, 0x7ffffff0, 1, 1), (1600, 64, 100, 64), (64, 1600, 64, 100)):
        plan.value = 0x1000
        assert lib.mulut_resample_plan_create(0, *dims, ctypes.byref(plan)) == EUNSUPPORTED and not plan.value
    assert lib.mulut_resample_plan_destroy(None) == EINVAL
    HWC = 1
    for args in ((None, 0x1000, HWC, 0x2000, HWC, 1, 3), (0x3000, None, HWC, 0x2000, HWC, 1, 3), (0x3000, 0x1000, HWC, None, HWC, 1, 3),
                 (0x3000, 0x1000, HWC, 0x2000, HWC, 0, 3), (0x3000, 0x1000, HWC, 0x2000, HWC, -1, 3),
                 (0x3000, 0x1000, HWC, 0x2000, HWC, 1, 0), (0x3000, 0x1000, HWC, 0x2000, HWC, 1, -1)):
        assert lib.mulut_resample_run(*args, None) == EINVAL
    assert lib.mulut_version() == 100


def test_driver_flags_default_off(tmp_path):
    from mulut_amd import finetune_lut
    from mulut_amd.options import TestOptions
    assert finetune_lut.build_parser().parse_args(["-e", str(tmp_path)]).makeLR is False
    assert finetune_lut.build_parser().parse_args(["-e", str(tmp_path), "--makeLR"]).makeLR is True
    assert TestOptions().parse(["-e", str(tmp_path)]).bicubicBaseline is False
    assert TestOptions().parse(["-e", str(tmp_path), "--bicubicBaseline"]).bicubicBaseline is True


def test_lr_paths_are_the_reference_scripts_and_the_test_scripts():
    from mulut_amd.resample import lr_path, tile_w
    assert lr_path("root", "0001", 4, "div2k") == os.path.join("root", "LR", "X4", "0001x4.png")
    assert lr_path("root", "baby", 3, "benchmark") == os.path.join("root", "LR_bicubic", "X3", "baby.png")
    with pytest.raises(ValueError):
        lr_path("root", "baby", 3, "other")
    assert [tile_w(c) for c in (1, 2, 3, 4, 5)] == [256, 128, 84, 64, 256]


def test_host_half_as_a_program_under_sanitizers(tmp_path):
    """mulut_resample.hip's host half + fake_hip.cpp + resample_host.cpp (its own main), -fsanitize=address,undefined, run as a
    program: plan create / run / destroy with their allocations, copies and launch configurations, the refusals, the sweep."""
    from mulut_amd import _native
    import host_abi as tool
    if _native._hipcc() is None:
        pytest.skip("no hipcc")
    assert "mulut_resample.hip" in _native.SOURCES
    assert {"mulut_resample_coeffs", "mulut_resample_plan_create", "mulut_resample_plan_destroy", "mulut_resample_run"} <= set(_native.EXPORTS)
    r = tool.run(tool.build(str(tmp_path), tool.CSRC, "resample_host", ["mulut_resample.hip"]))
    print(r.stdout)
    assert r.stderr == "", r.stderr[-4000:]
    assert r.returncode == 0 and "UNEXPECTED" not in r.stdout and r.stdout.endswith("\n0 unexpected\n")
    lines = r.stdout.splitlines()
    assert "plan 1356 x 2040 -> 339 x 510 -> 0 [malloc 62484 | memcpy 62484]" in lines
    assert "run HWC C 3 -> 0 [launch resample_kernel<3> grid 154,1,1 block 256,1,1 lds 36864]" in lines
    assert "destroy -> 0 [free 62484]" in lines
    assert "%d axes swept" % len(list(_axes())) in lines
    assert sum(" -> -1 []" in ln for ln in lines) == 26 and sum(" -> -5 []" in ln for ln in lines) == 8 and "plan device 3 -> -7 []" in lines
