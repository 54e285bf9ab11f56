"""The fine-tune kernels order the four keys of a pass by ranks computed from comparisons (mulut_amd/csrc/mulut_ft.h: ft_order_code, the
one definition the kernels of every interval use) instead of the reference's 24-branch cascade of strict '>' tests (sr/model.py:191-282).
Gradients depend on the order at TIES, so the two must agree for every tie pattern: checked here exhaustively on a restatement of both
and on the function itself, compiled by g++ (tests/host_emul/emul_ft_interval.cpp).  The kernels themselves are held to reference-made
fixtures with integer inputs -- ties everywhere -- in tests/test_gpu_finetune.py."""
import ctypes
import itertools

import numpy as np

from host_emul_lib import load_emul_ft_interval


def cascade(fa, fb, fc, fd):
    """sr/model.py:191-282: the simplex case by strict comparisons, as the order of the key ids 0..3 (first = largest f)"""
    fab, fac, fad, fbc, fbd, fcd = fa > fb, fa > fc, fa > fd, fb > fc, fb > fd, fc > fd
    if fab and fbc:
        return (0, 1, 2, 3) if fcd else (0, 1, 3, 2) if fbd else (0, 3, 1, 2) if fad else (3, 0, 1, 2)
    if fab and fac:
        return (0, 2, 1, 3) if fbd else (0, 2, 3, 1) if fcd else (0, 3, 2, 1) if fad else (3, 0, 2, 1)
    if fab:
        return (2, 0, 1, 3) if fbd else (2, 0, 3, 1) if fad else (2, 3, 0, 1) if fcd else (3, 2, 0, 1)
    if fac:
        return (1, 0, 2, 3) if fcd else (1, 0, 3, 2) if fad else (1, 3, 0, 2) if fbd else (3, 1, 0, 2)
    if fbc:
        return (1, 2, 0, 3) if fad else (1, 2, 3, 0) if fcd else (1, 3, 2, 0) if fbd else (3, 1, 2, 0)
    return (2, 1, 0, 3) if fad else (2, 1, 3, 0) if fbd else (2, 3, 1, 0) if fcd else (3, 2, 1, 0)


def by_ranks(f):
    """ft_order_code: rank_i = #{j > i: f_j >= f_i} + #{j < i: f_j > f_i}; returns the key ids by rank"""
    lt = lambda x, y: int(x < y)      # noqa: E731  (the kernel: sign bit of the int32 difference of the float patterns)
    a, b, c, d = f
    s10, s20, s30, s21, s31, s32 = lt(b, a), lt(c, a), lt(d, a), lt(c, b), lt(d, b), lt(d, c)
    ranks = (3 - s10 - s20 - s30, s10 + 2 - s21 - s31, s20 + s21 + 1 - s32, s30 + s31 + s32)
    assert sorted(ranks) == [0, 1, 2, 3]
    code = (1 << (2 * ranks[1])) | (2 << (2 * ranks[2])) | (3 << (2 * ranks[3]))
    return tuple((code >> (2 * j)) & 3 for j in range(4))


def test_rank_order_equals_the_reference_cascade_for_every_tie_pattern():
    n = 0
    for f in itertools.product(range(4), repeat=4):      # four levels: every ordering and every tie pattern of four values
        assert by_ranks(f) == cascade(*f), f
        n += 1
    assert n == 256
    for f in itertools.product((0.0, 0.5, 7.25, 15.999), repeat=4):
        assert by_ranks(f) == cascade(*f), f


def test_compiled_order_code_equals_the_reference_cascade_for_every_tie_pattern():
    """ft_order_code as the kernels compile it (sign bits of int32 differences of the float patterns), on the same cases"""
    cases = list(itertools.product((0.0, 1.0, 2.0, 3.0), repeat=4)) + list(itertools.product((0.0, 0.5, 7.25, 15.999), repeat=4))
    cases += list(itertools.product((0.0, 1e-30, 31.5, 63.999), repeat=4))      # the smallest and the largest LSBs of any interval (q <= 64)
    f = np.ascontiguousarray(cases, np.float32)
    code = np.empty(len(f), np.int32)
    L = load_emul_ft_interval()
    L.emul_ft_order_code.restype = None
    L.emul_ft_order_code.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    L.emul_ft_order_code(f.ctypes.data, len(f), code.ctypes.data)
    assert len(f) == 3 * 256
    for row, c in zip(f, code):
        assert tuple((int(c) >> (2 * j)) & 3 for j in range(4)) == cascade(*row.tolist()), row
