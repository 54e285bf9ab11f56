"""What tests/test_net_exact_cpu.py and tests/test_gpu_net_exact.py share: the op-level models, shapes and gradient bar of
tests/net_train_cases.py, unchanged, and a NumPy / ctypes binding of the host model of the gather-form input gradient
(tests/host_emul/net_gx_host.cpp: the definition of mulut_net_gx_gather in include/mulut.h as scatter loops in its order).

The shapes of net_train_cases are already the smallest at which the gather can go wrong: one site; rows / columns shorter than every
pad, where every tap of a row collapses onto one pixel; plane boundaries inside a tile; one past a 32- and a 128-site tile each way.
"""
import ctypes

import numpy as np

from host_emul_lib import load_emul
from net_train_cases import C, OP_MODELS, OP_SHAPES, meets, model_id, op_case      # noqa: F401  (re-exported: the cases of the tests)

LETTERS = "sdyeho"
TS_ROUND = 128      # a pass's tap buffer is float [4][ts], ts its sites rounded up to this
_lib = []


def host():
    if not _lib:
        lib = load_emul("net_gx_host", [], ["-ffp-contract=off", "-DNET_GX_NO_MAIN"])
        fp, i = ctypes.POINTER(ctypes.c_float), ctypes.c_int
        lib.net_gx_host_pass.argtypes = [ctypes.c_char, i, fp, ctypes.c_longlong, i, i, i, i, fp, i]
        lib.net_gx_host_stage.argtypes = [ctypes.c_char_p, fp, ctypes.c_longlong, i, i, i, i, fp]
        lib.net_gx_host_pass.restype = lib.net_gx_host_stage.restype = i
        _lib.append(lib)
    return _lib[0]


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def host_pass(mode, r, t, shape, gx=None):
    """gx (float32 [N, C, H, W]) of one pass from t (float32 [4, ts]): written when gx is None, else added to a copy of gx."""
    assert t.dtype == np.float32 and t.ndim == 2 and t.shape[0] == 4 and t.flags.c_contiguous and t.shape[1] >= int(np.prod(shape))
    out = np.full(shape, np.nan, np.float32) if gx is None else np.ascontiguousarray(gx, np.float32).copy()
    assert host().net_gx_host_pass(mode.encode(), r, _fp(t), t.shape[1], *shape, _fp(out), int(gx is not None)) == 0
    return out


def host_stage(modes, t, shape):
    """gx of a stage from t (float32 [4 M, 4, ts]): the passes in the backward's order, the first written, the others added."""
    assert t.dtype == np.float32 and t.shape[:2] == (4 * len(modes), 4) and t.flags.c_contiguous and t.shape[2] >= int(np.prod(shape))
    out = np.full(shape, np.nan, np.float32)
    assert host().net_gx_host_stage(modes.encode(), _fp(t), t.shape[2], *shape, _fp(out)) == 0
    return out


def mixed_taps(rng, passes, ts):
    """float32 [passes, 4, ts]: standard normal times 2^e, e drawn in -20..20 per element -- a sum of such terms depends, in its last
    bits, on the order of the adds."""
    return (rng.standard_normal((passes, 4, ts)) * np.exp2(rng.integers(-20, 21, (passes, 4, ts)))).astype(np.float32)
