#!/usr/bin/env python3
"""The library's host layer on the CPU: what every C-ABI call asks of the HIP runtime, without a GPU.

  tools/host_abi.py build OUTDIR [--csrc DIR]     the host half of every file of _native.SOURCES (hipcc --cuda-host-only, the warning
                                                  flags of _native.HIPCC_FLAGS, -fsanitize=address,undefined) linked with
                                                  tests/host_emul/fake_hip.cpp and abi_host.cpp into OUTDIR/abi_host; DIR defaults
                                                  to mulut_amd/csrc (a checkout of another commit: DIR = <checkout>/mulut_amd/csrc,
                                                  its include/mulut.h is found beside it)
  tools/host_abi.py trace OUTDIR [--csrc DIR]     build, run, print the trace (tests/golden/host_abi_trace.txt is this output for
                                                  the parent of the commit that last touched it)
  --driver abi_tables_host                        the same build around tests/host_emul/abi_tables_host.cpp, the driver of
                                                  mulut_read_table_image (its trace: tests/golden/host_tables_trace.txt)

The program is stand-alone (its own main, no LD_PRELOAD, nothing loaded into python): AddressSanitizer and
UndefinedBehaviorSanitizer watch the host code while it runs, LeakSanitizer reports at exit what was never freed.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EMUL = os.path.join(ROOT, "tests", "host_emul")
CSRC = os.path.join(ROOT, "mulut_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def build(outdir, csrc, driver="abi_host", sources=None, flags=()):
    """`sources`: the files of _native.SOURCES to compile (None: all of them); `flags`: more compile flags for every file of the program."""
    from mulut_amd import _native
    hipcc = _native._hipcc()
    sources = _native.SOURCES if sources is None else list(sources)
    outdir = os.path.abspath(outdir)
    os.makedirs(outdir, exist_ok=True)
    warn = [f for f in _native.HIPCC_FLAGS if f.startswith("-W") or f.startswith("-std")]
    host = [hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g"] + list(flags) + warn + ["-Xarch_host " + f for f in SAN]
    host = [x for f in host for x in f.split(" ")]
    jobs = [(s, subprocess.Popen(host + ["-c", "-o", os.path.join(outdir, s[:-4] + ".o"), s], cwd=csrc)) for s in sources]
    # (the two files of the harness always compile against THIS tree's include/mulut.h, whatever --csrc names: comparing two trees
    # this way presumes that the ABI header did not change between them)
    for s in ("fake_hip.cpp", driver + ".cpp"):
        jobs.append((s, subprocess.Popen(host + ["-x", "hip", "-c", "-o", os.path.join(outdir, s[:-4] + ".o"), os.path.join(EMUL, s)])))
    bad = [s for s, p in jobs if p.wait() != 0]
    if bad:
        sys.exit("failed to compile: %s" % " ".join(bad))
    exe = os.path.join(outdir, driver)
    objs = [os.path.join(outdir, s.rsplit(".", 1)[0] + ".o") for s, _ in jobs]
    clang = os.path.join(subprocess.check_output([os.path.join(os.path.dirname(hipcc), "hipconfig"), "-l"], text=True).strip(), "clang++")
    # (the per-file __hip_fatbin_* symbols of a host-only compile stay undefined: nothing reads them here)
    subprocess.check_call([clang] + SAN + ["-Wl,--unresolved-symbols=ignore-all", "-o", exe] + objs)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe] + list(args), env=env, capture_output=True, text=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cmd", choices=["build", "trace"])
    ap.add_argument("outdir")
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("--driver", default="abi_host", help="a driver of tests/host_emul, without its .cpp")
    args = ap.parse_args()
    exe = build(args.outdir, args.csrc, args.driver)
    if args.cmd == "trace":
        r = run(exe)
        sys.stderr.write(r.stderr)
        sys.stdout.write(r.stdout)
        sys.exit(r.returncode)
