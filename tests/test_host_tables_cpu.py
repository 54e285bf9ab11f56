"""mulut_read_table_image's host half on the CPU: tests/host_emul/abi_tables_host.cpp drives it beside mulut_set_lut through the
real C ABI, linked with the host half of every source file and the fake HIP runtime of tests/host_emul/fake_hip.cpp, as a
stand-alone program under AddressSanitizer, UndefinedBehaviorSanitizer and LeakSanitizer (tools/host_abi.py --driver
abi_tables_host; never loaded into Python).

tests/golden/host_tables_trace.txt is what the program printed when the accessor was written.  Beyond holding the program to it,
the header's contract is asserted on the trace itself, so that a regenerated golden file cannot hide a broken promise."""
import os
import re
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    from mulut_amd import _native
    import host_abi as tool
    if _native._hipcc() is None:
        pytest.skip("no hipcc")
    exe = tool.build(str(tmp_path_factory.mktemp("host_tables")), tool.CSRC, driver="abi_tables_host")
    r = tool.run(exe)
    assert r.stderr == "", r.stderr[-4000:]       # no sanitizer report, the leak check at exit included
    assert r.returncode == 0
    return r.stdout


def blocks(text):
    """[(call, rc, [event, ...])] with folded runs unfolded"""
    out = []
    for line in text.splitlines():
        m = re.match(r"^(\S.*) -> (-?\d+)$", line)
        if m:
            out.append((m.group(1), int(m.group(2)), []))
        elif line.startswith("  "):
            f = re.match(r"^  (.*) x(\d+)$", line)
            out[-1][2].extend([f.group(1)] * int(f.group(2)) if f else [line[2:]])
    return out


def test_program_keeps_its_trace(trace):
    want = open(os.path.join(GOLDEN, "host_tables_trace.txt")).read()
    assert len(want) < 100 * 1024
    got, exp = trace.splitlines(), want.splitlines()
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g == e, "line %d: got %r, expected %r (after %r)" % (k + 1, g, e, got[max(0, k - 5):k])
    assert len(got) == len(exp)


def test_a_read_waits_for_its_stream_and_copies_what_was_asked(trace):
    """the size is that of the allocation mulut_set_lut made for the image; an image the slot does not have copies nothing"""
    last_set, reads = {}, 0
    for call, rc, ev in blocks(trace):
        if call.startswith("create"):      # a new context per interval: every slot empty
            last_set = {}
        m = re.match(r"^set_lut iv\d s(\d) (\w) v\d+ ", call)
        if m:
            last_set[(m.group(1), m.group(2))] = [int(e.split(" ")[1]) for e in ev if e.startswith("malloc ")] if any(
                e.startswith("malloc ") for e in ev) else last_set[(m.group(1), m.group(2))]
        m = re.match(r"^read_table_image s(\d) (\w) image (\d), 64 bytes$", call)
        if m:
            reads += 1
            sizes = last_set.get((m.group(1), m.group(2)), [])
            assert rc == (sizes[int(m.group(3))] if int(m.group(3)) < len(sizes) else 0), (call, rc, sizes)
            assert ev == (["wait stream", "memcpy 64"] if rc else ["wait stream"]), (call, ev)
    assert reads == 3 * (16 + 2) * 3


def test_sizes_of_every_shape(trace):
    sizes = {}
    for call, rc, ev in blocks(trace):
        m = re.match(r"^read_table_image s(\d) (\w) image (\d), 64 bytes$", call)
        if m and rc:
            sizes.setdefault((int(m.group(1)), m.group(2), int(m.group(3))), []).append(rc)
    # interval 4 first: stages 1..4 hold s tables of v 1, 4, 9, 16, stages 5..8 e tables
    assert [sizes[(s, "s", 0)][0] for s in (1, 2, 3, 4)] == [83536, 334084, 1002252, 1336336]
    assert [sizes[(s, "s", 1)][0] for s in (1, 2, 3, 4)] == [4176, 8336, 24992, 33312] and sizes[(4, "s", 2)][0] == 2516480
    assert sizes[(8, "e", 0)][0] == 1336336 and (8, "e", 1) not in sizes and (3, "s", 2) not in sizes
    assert 104976 in sizes[(4, "s", 0)] and 625 * 12 + 4 in sizes[(3, "s", 0)]      # intervals 5 and 6: padded plain rows


def test_refused_calls_return_their_code_and_touch_nothing(trace):
    codes = {"no context": -1, "image 3": -1, "image -1": -1, "no buffer": -1, "negative size": -1, "stage 0": -1, "stage 9": -1, "pattern q": -2}
    seen = set()
    for call, rc, ev in blocks(trace):
        if call.startswith("refused: "):
            seen.add(call[9:])
            assert rc == codes[call[9:]] and ev == [], (call, rc, ev)
    assert seen == set(codes)


def test_destroy_frees_everything(trace):
    mallocs, frees = [], []
    for call, rc, ev in blocks(trace):
        mallocs += [e.split(" ")[1] for e in ev if e.startswith("malloc ")]
        frees += [e.split(" ")[1] for e in ev if e.startswith("free ")]
        assert "free of an unknown pointer" not in ev, call
    assert sorted(mallocs) == sorted(frees) and len(mallocs) > 30
