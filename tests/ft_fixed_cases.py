"""Cases of the bit-reproducible (fixed-point) backward, mulut_ft_exact_stage_backward, and the host model they are held to (test
infrastructure, shared by test_ft_fixed_cpu.py and test_gpu_ft_fixed.py).

The reference of the GPU tests is tests/host_emul/ft_exact_host.cpp: the arithmetic of mulut_amd/csrc/mulut_ft_exact.h compiled by
g++ and walked site by site with plain int64 adds (a program of its own, built here under AddressSanitizer and
UndefinedBehaviorSanitizer).  The CPU tests hold that model to oracle/ft_torch.py's autograd; the GPU tests ask the kernels for the
model's BYTES.  Unlike tests/ft_exact_cases.py -- integer data chosen so that float sums are exact in any order -- the data here is
what the float kernels cannot reproduce: x mixes integer levels with float32(b / 255) * 255 values (stage 1's real inputs), the masks
are random, and grad_out has zeros, both signs and magnitudes spread over 2^-30 .. 1 of its maximum.
"""
import atexit
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
from host_abi import SAN      # noqa: E402  (the sanitizer flags of every stand-alone host program)

MAGIC = 0x46584331
HOST_SRC = os.path.join(ROOT, "tests", "host_emul", "ft_exact_host.cpp")
HOST_FLAGS = ["-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + SAN
ORDERS = {"ascending": 0, "descending": 1, "shuffled": 2}


def rows_of(interval):
    return (2 ** (8 - interval) + 1) ** 4


class Case:
    """One call.  kind: 'mixed' (the data described above) or 'headroom' (a constant image, every mask bit set, every grad_out equal to
    its maximum with the sign `sign`: the largest sum one table accumulator can receive at the shape)."""

    def __init__(self, tag, interval, u, last, modes, shape, kind="mixed", sign=1):
        self.interval, self.u, self.last, self.modes, self.shape, self.kind, self.sign = interval, u, last, modes, tuple(shape), kind, sign
        self.M = len(modes)
        self.name = "%s_iv%d_u%d_%s_%s" % (tag, interval, u, modes, "x".join(str(v) for v in shape))
        self.tables = self.x = self.gout = self.inside = None

    @property
    def avg(self):
        return self.M if self.last else 4 * self.M

    def build(self):
        if self.x is not None:
            return self
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        B, C, H, W = self.shape
        u, el = self.u, self.u * self.u
        self.tables = rng.integers(-127, 128, (self.M, rows_of(self.interval), el)).astype(np.float32)
        if self.kind == "headroom":
            self.x = np.full(self.shape, 128.0, np.float32)      # LSB 0 at every interval: all the weight of a pass on one row
            self.gmax = np.nextafter(np.float32(2.0), np.float32(0.0))      # just below a power of two: the most bits a scale leaves
            self.gout = np.full((B, C, H * u, W * u), self.sign * self.gmax, np.float32)
            self.inside = np.full(self.shape, (1 << el) - 1, np.uint16)
            return self
        levels = rng.integers(0, 256, self.shape)
        bytes_ = rng.integers(0, 256, self.shape)
        frac = (bytes_.astype(np.float32) / np.float32(255)) * np.float32(255)      # what the module's x * 255 gives stage 1
        self.x = np.where(rng.random(self.shape) < 0.5, levels.astype(np.float32), frac).astype(np.float32)
        n = (B, C, H * u, W * u)
        self.gmax = np.float32(3.7e-3)
        mag = (self.gmax * np.exp2(-30.0 * rng.random(n))).astype(np.float32)
        g = mag * rng.choice(np.array([-1.0, 1.0], np.float32), n)
        g[rng.random(n) < 0.15] = 0.0
        g.reshape(-1)[int(rng.integers(0, g.size))] = -self.gmax      # the maximum is there, whatever was drawn
        self.gout = g.astype(np.float32)
        self.inside = rng.integers(0, 1 << 16, self.shape).astype(np.uint16)      # bits 0 .. u*u-1 count, the others must be ignored
        if B * C * H * W > 4:
            self.inside.reshape(-1)[:2] = [0, 0xFFFF]
        return self

    def free(self):
        """drop the arrays (a parametrised run keeps every Case alive)"""
        self.tables = self.x = self.gout = self.inside = None

    def mask_hr(self):
        """the mask as a [B, C, H*u, W*u] array of 0 / 1: bit sy*u+sx of site (y, x) at (y*u+sy, x*u+sx)"""
        B, C, H, W = self.shape
        u = self.u
        m = np.zeros((B, C, H, u, W, u), np.float64)
        for eo in range(u * u):
            m[:, :, :, eo // u, :, eo % u] = (self.inside >> eo) & 1
        return m.reshape(B, C, H * u, W * u)


def _cases():
    out = [Case("E1", 4, 1, 0, "sdy", (2, 2, 13, 11)),
           Case("E2", 4, 4, 1, "sdy", (2, 1, 9, 14)),
           Case("E3", 4, 2, 1, "sdy", (1, 3, 7, 5)),
           Case("E3", 4, 3, 1, "sdy", (1, 3, 7, 5))]
    for iv in (5, 6):
        out += [Case("E4", iv, 1, 0, "sdy", (2, 2, 13, 11)), Case("E4", iv, 4, 1, "sdy", (2, 2, 13, 11))]
    for iv in (4, 5, 6):
        for modes in ("eho", "sdyeho"):
            out += [Case("E5", iv, 1, 0, modes, (1, 1, 8, 9)), Case("E5", iv, 4, 1, modes, (1, 1, 8, 9))]
        # every key clamps: the input gradient folds maximally
        out += [Case("E5", iv, 4, 1, "sdyeho", (1, 1, 1, 1)), Case("E5", iv, 1, 0, "sdyeho", (1, 1, 2, 3))]
    out += [Case("E6", 4, 1, 1, "s", (4, 1, 48, 48), "headroom", 1), Case("E6", 4, 4, 1, "s", (4, 1, 48, 48), "headroom", -1)]
    out += [Case("E8", 4, 1, 0, "sdy", (3, 1, 19, 23)), Case("E8", 4, 4, 1, "sdy", (3, 1, 19, 23))]      # 1,311 sites: six workgroups, the last partial
    assert len(set(c.name for c in out)) == len(out)
    return out


CASES = _cases()
HEADROOM = [c for c in CASES if c.kind == "headroom"]
E7 = Case("E7", 5, 2, 1, "sdy", (1, 2, 6, 7))      # prior contents of the destinations


_exe = []


def host_model():
    """the host model's program, built once per process"""
    if not _exe:
        d = tempfile.mkdtemp(prefix="ft_exact_host_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "ft_exact_host")
        subprocess.check_call(["g++"] + HOST_FLAGS + ["-o", exe, HOST_SRC])
        _exe.append(exe)
    return _exe[0]


class Expected:
    pass


def expected(case, order="ascending", seed=0, prior=None, perm=None):
    """What the call must leave in grad_wq ([M, rows, u*u]) and grad_x, by the host model; .gbits, .Sw, .Sx, .max_w, .max_x from its report.
    prior: (grad_wq, grad_x) held before the call; perm: the batch samples in this order."""
    case.build()
    B, C, H, W = case.shape
    x, gout, inside = case.x, case.gout, case.inside
    if perm is not None:
        x, gout, inside = x[list(perm)], gout[list(perm)], inside[list(perm)]
    per = rows_of(case.interval) * case.u * case.u
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<12i", MAGIC, case.interval, case.u, case.last, B, C, H, W, case.M, ORDERS[order], seed, int(prior is not None)))
            f.write(case.modes.encode().ljust(8, b"\0"))
            for a in (case.tables, x, gout):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
            f.write(np.ascontiguousarray(inside, np.uint16).tobytes())
            if prior is not None:
                f.write(np.ascontiguousarray(prior[0], np.float32).tobytes())
                f.write(np.ascontiguousarray(prior[1], np.float32).tobytes())
        r = subprocess.run([host_model(), src, dst], capture_output=True, text=True)
        assert r.returncode == 0, (case.name, r.returncode, r.stderr[-2000:])
        raw = np.fromfile(dst, np.float32)
    e = Expected()
    e.gw = raw[:case.M * per].reshape(case.M, -1, case.u * case.u)
    e.gx = raw[case.M * per:].reshape(case.shape)
    e.gbits, e.Sw, e.Sx, e.max_w, e.max_x = [int(v) for v in r.stdout.split()]
    return e
