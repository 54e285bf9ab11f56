"""The library's host layer on the CPU: the host half of every source file, linked against a fake HIP runtime
(tests/host_emul/fake_hip.cpp: device memory is malloc, launches are logged) and driven through the real C ABI by a stand-alone
program (tests/host_emul/abi_host.cpp) under AddressSanitizer, UndefinedBehaviorSanitizer and LeakSanitizer.

tests/golden/host_abi_trace.txt is what that program printed for the sources BEFORE the context's buffers got their owner type and
the fine-tune entry points their one dispatcher (`tools/host_abi.py trace OUT --csrc <that checkout>/mulut_amd/csrc`): every call's
return code, allocations, frees, copies, waits, events and launch configurations.  The host layer must keep printing it."""
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def host_abi(tmp_path_factory):
    from mulut_amd import _native
    import host_abi as tool
    if _native._hipcc() is None:
        pytest.skip("no hipcc")
    exe = tool.build(str(tmp_path_factory.mktemp("host_abi")), tool.CSRC)
    return tool, exe


def test_host_layer_keeps_its_trace_and_frees_what_it_takes(host_abi):
    tool, exe = host_abi
    r = tool.run(exe)
    assert r.stderr == "", r.stderr[-4000:]       # no sanitizer report, the leak check at exit included
    assert r.returncode == 0
    want = open(os.path.join(GOLDEN, "host_abi_trace.txt")).read()
    assert len(want) < 100 * 1024
    got, exp = r.stdout.splitlines(), want.splitlines()
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g == e, "line %d: got %r, expected %r (after %r)" % (k + 1, g, e, got[max(0, k - 5):k])
    assert len(got) == len(exp)


def test_leak_check_is_alive(host_abi):
    """The same program with its last context never destroyed: LeakSanitizer must say so, or the test above proves nothing here."""
    tool, exe = host_abi
    r = tool.run(exe, "--skip-destroy")
    assert r.returncode != 0
    assert "LeakSanitizer" in r.stderr and " leaked in " in r.stderr and "allocation(s)" in r.stderr, r.stderr[-2000:]
