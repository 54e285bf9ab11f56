"""Every compiled instance and store path of the fused SR-network kernels on the GPU (-m gpu), against float64.

The cases, the comparison (exact wherever float64 decides a value, the statistical bar of net_cases.py elsewhere) and where T comes
from: tests/net_grid_cases.py.  The gradient bar and the kink-free g: tests/net_train_cases.py.

  1. tables, passes, stages and stage sums of GRID_MODELS -- the (MT, U) instances (1, 4), (2, 2), (2, 3), a full single tile and a unit
     that is all padding -- and of the SEEDED models of test_gpu_net.py, on GRID_SHAPES;
  2. both backwards for the pairings of nf and u that change net_wgrad_pairs, net_ws_rows and the layer-6 tile, and a chunk loop of
     several workgroups per chunk with a short last chunk;
  3. the packed and the scalar store paths of mulut_net_table and mulut_net_stage through the C ABI, on pointers at every alignment
     include/mulut.h allows, between guard bytes;
  4. stages only the C ABI can express: MULUT_MAX_MODES units with repeated letters, and units of different nf under one padded width.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import net_cases as nc
import net_grid_cases as gc
import net_train_cases as tc
from test_gpu_net_exact import _raw_backward
from test_gpu_net_train import _sum_bar

pytestmark = pytest.mark.gpu

NF64_X4 = tc.OP_MODELS[1]
assert gc.pairs(NF64_X4) == [(2, 4)]
GUARD, LEAD = 0xEE, 32


def _lib():
    from mulut_amd import _native
    return _native.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _engine(cfg):
    from mulut_amd.net_engine import NetEngine
    return NetEngine(gc.nets(cfg)[0])


def _trainer(cfg, deterministic=False):
    from mulut_amd.net_train import NetTrainer
    tr = NetTrainer(copy.deepcopy(gc.nets(cfg)[0]).cuda(), deterministic=deterministic)
    tr.load(cfg["stages"])
    return tr


# ------------------------------------------------------------------------------------------------------------------ 1. the forward
@pytest.mark.parametrize("cfg", gc.GRID_MODELS, ids=tc.model_id)
def test_tables_at_intervals_5_and_6(cfg):
    """6,561 and 625 rows (a tail of 1 and of 113 rows past a 128-row workgroup) against the unit in float64 on the same grid."""
    net64 = gc.nets(cfg, "cuda")[1]
    eng, u = _engine(cfg), cfg["scale"]
    got, want = [], []
    for m in cfg["modes"]:
        for interval in (5, 6):
            t = eng.table(1, m, interval)
            assert t.dtype == torch.int8 and tuple(t.shape) == (((256 >> interval) + 1) ** 4, 1, u, u)
            v64 = gc.table_values(getattr(net64, "s1_" + m).model, interval).cpu().numpy()
            got.append(t.cpu().numpy().reshape(v64.shape).ravel())
            want.append(v64.ravel())
    gc.exact_where_decided(np.concatenate(got), np.concatenate(want), tc.model_id(cfg) + " tables at intervals 5 and 6")
    eng.close()


@pytest.mark.parametrize("cfg", gc.GRID_MODELS + gc.SEEDED, ids=tc.model_id)
def test_passes_stages_and_sums_where_float64_decides(cfg):
    """Every mode and rotation of every stage on GRID_SHAPES.  A pass value is round(v64) wherever v64 is decided; a stage byte and a
    stage sum are the float64 ones wherever all 4 M terms of the output are; elsewhere the bars of test_gpu_net.py and
    test_gpu_net_train.py hold.  The stage is the epilogue of the engine's own passes bit for bit, and two sums are equal."""
    eng, tr = _engine(cfg), _trainer(cfg)
    M = len(cfg["modes"])
    kinds = {k: ([], []) for k in ("passes", "stages", "sums")}
    open_outputs = outputs = 0
    for shape in gc.GRID_SHAPES:
        for s, (x, v64, last) in enumerate(gc.forward_case(cfg, shape, "cuda"), 1):
            what = "%s %r s%d" % (tc.model_id(cfg), shape, s)
            got_p = torch.stack([eng.pass_(s, m, r, x) for m in cfg["modes"] for r in range(4)]).cpu().numpy()
            out = eng.stage(s, x).cpu().numpy()
            xf = nc._unit_interval(x, torch.float32)
            tr.load(s)
            with torch.no_grad():
                p, again = tr.stage_sum(s, xf), tr.stage_sum(s, xf)
            assert torch.equal(p, again) and torch.equal(p, torch.round(p)), what
            sums = p.cpu().numpy().astype(np.int64)
            assert np.array_equal(out, nc.epilogue(got_p, last)), what
            want_p, full = gc.rounded(v64), gc.all_decided(v64)
            want_out, want_sum = nc.epilogue(want_p, last), want_p.sum(0)
            assert np.array_equal(out[full], want_out[full]), (what, "stage bytes where every term is decided")
            assert np.array_equal(sums[full], want_sum[full]), (what, "stage sums where every term is decided")
            open_outputs, outputs = open_outputs + int((~full).sum()), outputs + full.size
            for kind, g, w in (("passes", got_p, v64), ("stages", out, want_out), ("sums", sums, want_sum)):
                kinds[kind][0].append(g.ravel())
                kinds[kind][1].append(w.ravel())
    got, want = {k: np.concatenate(v[0]) for k, v in kinds.items()}, {k: np.concatenate(v[1]) for k, v in kinds.items()}
    undecided = gc.exact_where_decided(got["passes"], want["passes"], tc.model_id(cfg) + " passes")
    worst, share = nc.off(got["stages"], want["stages"])
    assert worst <= 1 and share <= 4 * M * nc.BAR, (worst, share)
    _sum_bar(got["sums"], want["sums"], M, tc.model_id(cfg) + " sums")
    print("%s: undecided values: passes %d of %d; stage bytes and sums with an undecided term %d of %d (stage bytes off %.3g)"
          % (tc.model_id(cfg), undecided, want["passes"].size, open_outputs, outputs, share))
    eng.close()
    tr.close()


# ----------------------------------------------------------------------------------------------------------------- 2. the backward
def _names(tr, stage):
    pn = {id(p): n for n, p in tr.model.named_parameters()}
    return [pn[id(p)] for p in tr.stage_params(stage)]


@pytest.mark.parametrize("cfg", gc.GRID_MODELS, ids=tc.model_id)
def test_both_backwards_of_the_new_pairings(cfg):
    """nf <= 32 with u = 4, nf > 32 with u = 2 and 3, nf 32 and nf 1: what test_backward_against_float64_on_the_same_inputs and
    test_exact_backward_at_op_level assert of their models."""
    plain, det = _trainer(cfg), _trainer(cfg, True)
    names, worst = _names(plain, 1), 0.0
    for shape in gc.GRID_SHAPES:
        case = tc.op_case(cfg, shape, 1, "cuda")
        assert case["dropped"] <= tc.MAX_DROP
        x, g = case["x"], case["g"]
        what = "%s %r" % (tc.model_id(cfg), shape)
        # the default path
        gx, gp = plain._backward(1, x, g, True)
        none, gp_none = plain._backward(1, x, g, False)
        _, gp_again = plain._backward(1, x, g, True)
        assert none is None
        for n, a, b, c in zip(names, gp, gp_none, gp_again):
            assert torch.equal(a, b) and torch.equal(a, c), (what, n)
            worst = max(worst, tc.meets(a, case["gp64"][n], what + " " + n))
        worst = max(worst, tc.meets(gx, case["gx64"], what + " gx"))
        # the deterministic path
        dgx, dgp = det._backward(1, x, g, True)
        dgx_again, _ = det._backward(1, x, g, True)
        small = det.workspace(1, x.numel(), min_sites=128)
        assert small.numel() == det._lib.mulut_net_backward_exact_ws_bytes(cfg["nf"], case["u"], 128, x.numel())
        dgx_small, dgp_small = det._backward(1, x, g, True, ws=small)
        worst = max(worst, tc.meets(dgx, case["gx64"], what + " gx (deterministic)"))
        assert torch.equal(dgx, dgx_again) and torch.equal(dgx, dgx_small), what
        for n, a, b, c in zip(names, dgp, gp, dgp_small):
            assert torch.equal(a, b), (what, n)
            worst = max(worst, tc.meets(c, case["gp64"][n], what + " " + n + " (smallest workspace)"))
        filled = torch.full_like(x, float("nan"))
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in det.stage_params(1)]
        _raw_backward(det, 1, x, g, filled, det.workspace(1, x.numel()), grads)
        assert torch.isfinite(filled).all() and torch.equal(filled, dgx), what
    print("%s: largest distance %.3g (bar %.3g)" % (tc.model_id(cfg), worst, tc.C))
    plain.close()
    det.close()


@pytest.mark.parametrize("cfg", gc.GRID_MODELS + [NF64_X4], ids=tc.model_id)
def test_backward_in_chunks_of_several_workgroups_with_a_short_last_chunk(cfg):
    """1 x 1 x 33 x 65 = 2,145 sites over a workspace of 384: five chunks of three workgroups, then a chunk of 225 sites -- two
    workgroups, the second with 97 sites and 31 idle lanes.  net_wgrad_kernel must stop at the rows of those two workgroups: the third
    workgroup's rows hold what the chunk before left (the workspace starts as NaN bytes, so a row nobody wrote shows as well)."""
    shape = (1, 1, 33, 65)
    plain, det = _trainer(cfg), _trainer(cfg, True)
    names, worst = _names(plain, 1), 0.0
    case = tc.op_case(cfg, shape, 1, "cuda")
    x, g, sites = case["x"], case["g"], case["x"].numel()
    what = "%s %r in chunks of 384" % (tc.model_id(cfg), shape)
    ws = plain.workspace(1, sites, min_sites=384)
    assert ws.numel() == plain._lib.mulut_net_backward_ws_bytes(cfg["nf"], case["u"], 384) and sites == 5 * 384 + 128 + 97
    ws.fill_(0xFF)
    gx, gp = plain._backward(1, x, g, True, ws=ws)
    dws = det.workspace(1, sites, min_sites=384)
    assert dws.numel() == det._lib.mulut_net_backward_exact_ws_bytes(cfg["nf"], case["u"], 384, sites)
    dws.fill_(0xFF)
    dgx, dgp = det._backward(1, x, g, True, ws=dws)
    whole, _ = det._backward(1, x, g, True)
    for n, a, b in zip(names, gp, dgp):
        assert torch.equal(a, b), (what, n)      # (the same chunks, so the same partial sums)
        worst = max(worst, tc.meets(a, case["gp64"][n], what + " " + n))
    worst = max(worst, tc.meets(gx, case["gx64"], what + " gx"))
    assert torch.equal(dgx, whole), what
    print("%s: largest distance %.3g (bar %.3g)" % (what, worst, tc.C))
    plain.close()
    det.close()


# -------------------------------------------------------------------------------------------- 3. store paths and pointer offsets
def _guarded(nbytes, off):
    """(the whole allocation, its nbytes at byte offset `off` past a 32-byte boundary): everything GUARD."""
    buf = torch.full((LEAD + off + nbytes + LEAD,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, buf[LEAD + off:LEAD + off + nbytes]


def _guards_intact(buf, off, nbytes):
    return bool((buf[:LEAD + off] == GUARD).all()) and bool((buf[LEAD + off + nbytes:] == GUARD).all())


@pytest.mark.parametrize("cfg,offsets", [(gc.GRID_MODELS[0], (8, 1, 4)), (NF64_X4, (8, 1, 4)), (gc.GRID_MODELS[1], (1,)), (gc.GRID_MODELS[2], (1,))],
                         ids=lambda v: tc.model_id(v) if isinstance(v, dict) else "off" + "_".join(map(str, v)))
def test_table_rows_at_any_alignment(cfg, offsets):
    """u = 4 packs a row half into one 8-byte store when `rows` is 8-aligned (offset 8: the control) and stores bytes otherwise
    (offsets 1 and 4); u = 2 and 3 store bytes.  The same bytes as the aligned call, and nothing outside them."""
    eng, lib, u = _engine(cfg), _lib(), cfg["scale"]
    for m in cfg["modes"]:
        for interval in (5, 6):
            want = eng.table(1, m, interval).view(torch.uint8).reshape(-1)
            for off in offsets:
                buf, view = _guarded(want.numel(), off)
                assert view.data_ptr() % 8 == off % 8
                assert lib.mulut_net_table(eng._units.handle(1, m), interval, view.data_ptr(), _stream()) == 0
                assert torch.equal(view, want), (tc.model_id(cfg), m, interval, off, u)
                assert _guards_intact(buf, off, want.numel()), (tc.model_id(cfg), m, interval, off)
    eng.close()


@pytest.mark.parametrize("cfg,out_offsets", [(gc.GRID_MODELS[0], (4, 1, 2)), (NF64_X4, (4, 1, 2)), (gc.GRID_MODELS[2], (1,))],
                         ids=lambda v: tc.model_id(v) if isinstance(v, dict) else "off" + "_".join(map(str, v)))
def test_stage_bytes_at_any_alignment(cfg, out_offsets):
    """u = 4 packs a block row into one 4-byte store when `out` is 4-aligned (offset 4: the control) and stores bytes otherwise
    (offsets 1 and 2); u = 3 stores bytes; `in` at offset 1 is read byte by byte.  The same bytes as the aligned call."""
    eng, lib, u = _engine(cfg), _lib(), cfg["scale"]
    modes = cfg["modes"].encode()
    for shape in ((2, 3, 5, 7), (1, 1, 33, 65)):
        N, C, H, W = shape
        x = gc.input_bytes(cfg, shape).cuda()
        want = eng.stage(1, x).reshape(-1)
        for in_off, out_off in [(0, o) for o in out_offsets] + [(1, 0)]:
            xbuf, xin = _guarded(x.numel(), in_off)
            xin.copy_(x.reshape(-1))
            buf, view = _guarded(want.numel(), out_off)
            assert view.data_ptr() % 4 == out_off % 4 and xin.data_ptr() % 4 == in_off
            rc = lib.mulut_net_stage(eng._units.handles(1), modes, 1, xin.data_ptr(), view.data_ptr(), N, C, H, W, _stream())
            assert rc == 0
            assert torch.equal(view, want), (tc.model_id(cfg), shape, in_off, out_off, u)
            assert _guards_intact(buf, out_off, want.numel()) and _guards_intact(xbuf, in_off, x.numel()) and torch.equal(xin, x.reshape(-1))
    eng.close()


# ----------------------------------------------------------------------------------- 4. stage shapes only the C ABI can express
class _Units(object):
    """The training units of a spec of net_grid_cases.py (a list of (model, letters)) in its order, their parameters loaded."""

    def __init__(self, spec):
        self.modes = gc.multi_modes(spec)
        self.trainers = [_trainer(cfg) for cfg, _ in spec]
        self.units = [(k, tr, letter) for k, (tr, (_, letters)) in enumerate(zip(self.trainers, spec)) for letter in letters]
        self.M = len(self.units)
        self.handles = (ctypes.c_void_p * self.M)(*[tr._units.handle(1, letter).value for _, tr, letter in self.units])
        self.nf, self.u = spec[0][0]["nf"], spec[0][0]["scale"]

    def params(self):
        """per unit (model index, [names of conv1..conv6 weights, then biases], [the tensors])"""
        from mulut_amd.net_engine import unit_layers
        out = []
        for k, tr, letter in self.units:
            pn = {id(p): n for n, p in tr.model.named_parameters()}
            layers = unit_layers(getattr(tr.model, "s1_" + letter).model)
            tensors = [c.weight for c in layers] + [c.bias for c in layers]
            out.append((k, [pn[id(p)] for p in tensors], tensors))
        return out

    def close(self):
        for tr in self.trainers:
            tr.close()


def _forward_of_a_unit_list(spec, shape):
    lib, un, case = _lib(), _Units(spec), gc.multi_case(spec, shape, "cuda")
    N, C, H, W = shape
    u, xb, v64, what = case["u"], case["xb"], case["v64"], gc.multi_id(spec)
    passes = torch.empty((4 * un.M, N, C, H * u, W * u), dtype=torch.int8, device="cuda")
    for m, (_, tr, letter) in enumerate(un.units):
        for r in range(4):
            assert lib.mulut_net_pass(tr._units.handle(1, letter), letter.encode(), r, xb.data_ptr(), N, C, H, W, passes[4 * m + r].data_ptr(), _stream()) == 0
    out = torch.empty((N, C, H * u, W * u), dtype=torch.uint8, device="cuda")
    pred = torch.full((N, C, H * u, W * u), float("nan"), dtype=torch.float32, device="cuda")
    assert lib.mulut_net_stage(un.handles, un.modes.encode(), 1, xb.data_ptr(), out.data_ptr(), N, C, H, W, _stream()) == 0
    assert lib.mulut_net_stage_sum(un.handles, un.modes.encode(), case["x"].data_ptr(), N, C, H, W, pred.data_ptr(), _stream()) == 0
    got_p = passes.cpu().numpy()
    undecided = gc.exact_where_decided(got_p, v64, what + " passes")
    assert np.array_equal(out.cpu().numpy(), nc.epilogue(got_p, True)), what
    sums, full = pred.cpu().numpy(), gc.all_decided(v64)
    assert np.array_equal(sums, np.rint(sums)) and np.array_equal(sums[full], gc.rounded(v64).sum(0)[full]), what
    assert np.array_equal(sums[full], got_p.astype(np.int64).sum(0)[full]), what
    _sum_bar(sums.astype(np.int64), got_p.astype(np.int64).sum(0), un.M, what + " sums against passes")
    print("%s: undecided values: passes %d of %d; sums with an undecided term %d of %d" % (what, undecided, v64.size, int((~full).sum()), full.size))
    return lib, un, case


def _raw_backwards(lib, un, case, shape, modes=None, handles=None):
    """(rc, gx, grads per unit) of mulut_net_stage_backward and of _exact on the units of `un`."""
    N, C, H, W = shape
    sites, out = N * C * H * W, []
    params = un.params()
    M = len(params) if handles is None else len(handles)
    for exact in (False, True):
        nbytes = lib.mulut_net_backward_exact_ws_bytes(un.nf, un.u, sites, sites) if exact else lib.mulut_net_backward_ws_bytes(un.nf, un.u, sites)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        gx = torch.full_like(case["x"], float("nan")) if exact else torch.zeros_like(case["x"])
        grads = [[torch.full_like(p, float("nan"), memory_format=torch.contiguous_format) for p in tensors] for _, _, tensors in params]
        flat = [grads[m % len(grads)] for m in range(M)]
        gw = (ctypes.c_void_p * (6 * M))(*[flat[m][l].data_ptr() for m in range(M) for l in range(6)])
        gb = (ctypes.c_void_p * (6 * M))(*[flat[m][6 + l].data_ptr() for m in range(M) for l in range(6)])
        entry = lib.mulut_net_stage_backward_exact if exact else lib.mulut_net_stage_backward
        rc = entry(un.handles if handles is None else handles, (un.modes if modes is None else modes).encode(), case["x"].data_ptr(), case["g"].data_ptr(),
                   N, C, H, W, ws.data_ptr(), ws.numel(), gx.data_ptr(), gw, gb, _stream())
        out.append((rc, gx, grads))
    return out


def test_a_stage_of_eight_units_and_a_refusal_of_nine():
    """M = MULUT_MAX_MODES: "sdyehosd", the six units of one seeded nf 24 x2 model and s, d of another.  The stage is the epilogue of the
    32 passes exactly, the sum is theirs wherever decided, both backwards meet the gradient bar against float64 over the same eight
    units; a ninth unit is refused."""
    shape = (2, 3, 5, 7)
    lib, un, case = _forward_of_a_unit_list(gc.EIGHT, shape)
    assert un.M == 8 and un.modes == "sdyehosd" and case["dropped"] <= tc.MAX_DROP
    worst = 0.0
    (rc, gx, grads), (rc_x, gx_x, grads_x) = _raw_backwards(lib, un, case, shape)
    assert rc == 0 and rc_x == 0
    for (k, names, _), got, got_x in zip(un.params(), grads, grads_x):
        for n, a, b in zip(names, got, got_x):
            assert torch.equal(a, b), n
            worst = max(worst, tc.meets(a, case["gp64"][k][n], "eight units, model %d %s" % (k, n)))
    worst = max(worst, tc.meets(gx, case["gx64"], "eight units gx"), tc.meets(gx_x, case["gx64"], "eight units gx (deterministic)"))
    print("%s: largest distance %.3g (bar %.3g)" % (gc.multi_id(gc.EIGHT), worst, tc.C))
    # nine: refused by every stage call, before anything is launched
    nine = (ctypes.c_void_p * 9)(*([h for h in un.handles] + [un.handles[2]]))
    N, C, H, W = shape
    out = torch.full((N, C, H * 2, W * 2), GUARD, dtype=torch.uint8, device="cuda")
    pred = torch.full((N, C, H * 2, W * 2), 7.0, dtype=torch.float32, device="cuda")
    assert lib.mulut_net_stage(nine, b"sdyehosdy", 1, case["xb"].data_ptr(), out.data_ptr(), N, C, H, W, _stream()) == -5
    assert lib.mulut_net_stage_sum(nine, b"sdyehosdy", case["x"].data_ptr(), N, C, H, W, pred.data_ptr(), _stream()) == -5
    for rc9, gx9, _ in _raw_backwards(lib, un, case, shape, "sdyehosdy", nine):
        assert rc9 == -5
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()) and bool((pred == 7.0).all())
    un.close()


def test_units_of_different_nf_under_one_padded_width():
    """nf 8 and nf 24, both one feature tile, u = 2: the forward takes them (include/mulut.h asks for one u and one padded width),
    both backwards refuse them with MULUT_ESHAPE and write nothing."""
    shape = (2, 3, 5, 7)
    lib, un, case = _forward_of_a_unit_list(gc.MIXED, shape)
    assert un.M == 2 and len({tr._units.nf(1) for tr in un.trainers}) == 2
    for rc, gx, grads in _raw_backwards(lib, un, case, shape):
        assert rc == -4
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for unit in grads for t in unit)
    un.close()
