"""stage_u1t_kernel's one-hot neighbourhood test and one-operation sort keys on the device (-m gpu).  Crafted frames from
tests/k1_diet_cases.py (tests/test_k1_dirty_cpu.py asserts on the oracle alone what they hold: dirty and clean sites in every tile, and
bytes that change when a flag is missed) with the tube kernel on every tile: 70 x 134 HWC frames (two tile rows, three tile columns,
the last 6 pixels wide; W % 4 != 0 takes the kernel's byte path) and 66 x 128 planar ones (its dword path), as stage 1 alone and as
the 2-stage sdy x4 cascade, plus one case each on the x2 and x3 final-stage instances.
Bar: np.array_equal with oracle.c_oracle, no tolerance; where the kernel ran alone, the length of its fix-up list equals the
reference's number of dirty sites -- a missed or a spurious flag changes that number even where the bytes agree."""
import numpy as np
import pytest

import k1_diet_cases as K
from oracle import c_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from mulut_amd import MuLUTEngine  # noqa: E402
from mulut_amd.engine import LAYOUT_CHW, LAYOUT_HWC  # noqa: E402

POISON = 0xA5
SHAPES = {"hwc": (K.H_HWC, K.W_HWC, LAYOUT_HWC), "planar": (K.H_PL, K.W_PL, LAYOUT_CHW)}


def dev(x_nhwc, layout):
    x = x_nhwc if layout == LAYOUT_HWC else x_nhwc.transpose(0, 3, 1, 2)
    return torch.from_numpy(np.array(x, order="C", copy=True)).cuda()


def host(t, layout):
    a = t.cpu().numpy()
    return a if layout == LAYOUT_HWC else a.transpose(0, 2, 3, 1)


def poisoned(n, h, w, c, layout):
    """an output buffer no earlier call's correct bytes are left in"""
    return torch.full((n, h, w, c) if layout == LAYOUT_HWC else (n, c, h, w), POISON, dtype=torch.uint8, device="cuda")


def engine(stages, scale, luts):
    """A context with the tube kernel on every tile of the first and of the x2 / x3 final stage.  last_detail_counters() reads the
    control block of the detailed-tile path, which a context allocates with its first hybrid x4 launch on planar input: one such
    launch first, whatever the configuration asked for."""
    e = MuLUTEngine(0).configure(2, "sdy", 4, 4).set_lut_dict(K.seeded_luts())
    e.stage(2, torch.full((3, 16, 64), 128, dtype=torch.uint8, device="cuda"), layout=LAYOUT_CHW, out_layout=LAYOUT_HWC)
    e.configure(stages, "sdy", scale, 4).set_lut_dict(luts)
    e.set_tuning("first_stage_detail_per_1024", 1024)
    e.set_tuning("final_stage_detail_per_1024", 1024)
    return e


def run_stage(e, s, x, layout):
    n, h, w, c = x.shape
    u = e.scale if s == e.stages else 1
    out = poisoned(n, h * u, w * u, c, layout)
    e.stage(s, dev(x, layout), layout=layout, out_layout=layout, out=out)
    return host(out, layout)


def run_pipeline(e, x, layout):
    n, h, w, c = x.shape
    out = poisoned(n, h * e.scale, w * e.scale, c, layout)
    e.pipeline(dev(x, layout), layout=layout, out=out)
    return host(out, layout)


def n_dirty(x):
    return int(sum(K.dirty_mask(f).sum() for f in x))


@pytest.fixture(scope="module")
def x4(shipped_luts):
    out = {}
    for kind, luts in (("shipped", shipped_luts), ("seeded", K.seeded_luts())):
        out[kind] = (engine(2, 4, luts), luts)
    yield out
    for e, _ in out.values():
        e.close()


@pytest.mark.parametrize("kind", ["shipped", "seeded"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_first_stage_alone_and_in_the_cascade(x4, name, shape, kind):
    e, luts = x4[kind]
    h, w, layout = SHAPES[shape]
    x = K.frames(name, h, w)
    assert "stage_u1t_kernel" in e.kernel_name(False), e.kernel_name(False)
    t1 = [luts["s1_%s" % m] for m in "sdy"]
    want1 = np.stack([c_oracle.stage(t1, "sdy", False, f, 1) for f in x])
    got1 = run_stage(e, 1, x, layout)
    fix, ref = e.last_detail_counters()["fix_pixels"], n_dirty(x)
    print(name, shape, kind, "stage 1: differing bytes", int((got1 != want1).sum()), "fix-up entries", fix, "reference dirty sites", ref)
    assert np.array_equal(got1, want1)
    assert fix == ref, (fix, ref)
    want = np.stack([c_oracle.pipeline(luts, 2, "sdy", 4, f) for f in x])
    got = run_pipeline(e, x, layout)
    print(name, shape, kind, "cascade: differing bytes", int((got != want).sum()))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_x2_final_stage_on_the_benchmarks_tables(shape):
    """stage_u1t_kernel<2> (4-value rows): the final stage of the benchmark's 4-stage x2 cascade alone, then the whole cascade (three
    1-byte-row stages in front of it)."""
    luts = K.config5_luts()
    e = engine(4, 2, luts)
    h, w, layout = SHAPES[shape]
    x = K.frames("isolated", h, w)
    assert "stage_u1t_kernel<2>" in e.kernel_name(True), e.kernel_name(True)
    want4 = np.stack([c_oracle.stage([luts["s4_%s" % m] for m in "sdy"], "sdy", True, f, 2) for f in x])
    got4 = run_stage(e, 4, x, layout)
    fix, ref = e.last_detail_counters()["fix_pixels"], n_dirty(x)
    print("x2", shape, "final stage: differing bytes", int((got4 != want4).sum()), "fix-up entries", fix, "reference dirty sites", ref)
    assert np.array_equal(got4, want4)
    assert fix == ref, (fix, ref)
    want = np.stack([c_oracle.pipeline(luts, 4, "sdy", 2, f) for f in x])
    got = run_pipeline(e, x, layout)
    print("x2", shape, "cascade: differing bytes", int((got != want).sum()))
    assert np.array_equal(got, want)
    e.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_x3_final_stage(shape):
    """stage_u1t_kernel<3> (9-value rows) as a single-stage x3 cascade on seeded tables"""
    luts = K.final_luts(3, 7)
    e = engine(1, 3, luts)
    h, w, layout = SHAPES[shape]
    x = K.frames("edges", h, w)
    assert "stage_u1t_kernel<3>" in e.kernel_name(True), e.kernel_name(True)
    want = np.stack([c_oracle.pipeline(luts, 1, "sdy", 3, f) for f in x])
    got = run_pipeline(e, x, layout)
    fix, ref = e.last_detail_counters()["fix_pixels"], n_dirty(x)
    print("x3", shape, "differing bytes", int((got != want).sum()), "fix-up entries", fix, "reference dirty sites", ref)
    assert np.array_equal(got, want)
    assert fix == ref, (fix, ref)
    e.close()
