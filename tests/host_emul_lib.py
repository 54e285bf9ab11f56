"""Builds (g++) and loads one of the CPU harnesses of tests/host_emul: shared source of the kernels compiled for the host, TEST ONLY."""
import ctypes
import os
import subprocess

from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "host_emul")


def load_emul(name, headers, flags=()):
    """tests/host_emul/<name>.cpp -> lib<name>.so (rebuilt when the source or one of the mulut_amd/csrc `headers` is newer), as a ctypes handle"""
    so, src = os.path.join(HERE, "lib%s.so" % name), os.path.join(HERE, name + ".cpp")
    deps = [src] + [os.path.join(ROOT, "mulut_amd", "csrc", h) for h in headers]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17"] + list(flags) + ["-fPIC", "-shared", "-Wall", "-o", so, src])
    return ctypes.CDLL(so)


def load_emul_ft_interval():
    """the fine-tune harness (mulut_ft.h, mulut_ft_interval.h): -ffp-contract=off, as the kernels are compiled (the reference's float expressions are not contracted)"""
    return load_emul("emul_ft_interval", ["mulut_core.h", "mulut_ft.h", "mulut_ft_interval.h"], ["-ffp-contract=off"])
