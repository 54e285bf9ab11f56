#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 assembly of two source trees ("did this kernel change?"), without a GPU.

  tools/asm_compare.py emit OUTDIR [--csrc DIR]          every file of _native.SOURCES -> OUTDIR/<name>.s, compiled with
                                                         _native.HIPCC_FLAGS minus -fPIC -shared, plus --cuda-device-only -S
                                                         (what audit_tube2_isa() does); DIR defaults to mulut_amd/csrc
  tools/asm_compare.py compare OLD_DIR NEW_DIR [--rename OLD=NEW ...] [--only FILE ...]
                                                         one line per kernel: identical | mnemonics | DIFFERENT, the instruction
                                                         counts and num_vgpr / numbered_sgpr / private_seg_size of both sides
  tools/asm_compare.py cut FILE.s MANGLED_NAME           the kernel's text, label to .Lfunc_end (tools/asm_stats.sh uses it)

A kernel's text is what lies between its label and its .Lfunc_end; comments, directives and blank lines are dropped and the
.LBB labels renumbered in order of appearance, so neither file names nor the position of a kernel in its file enter.  Kernels are
paired by demangled name without the argument list (a renamed argument struct or a move to another file does not unpair them);
--rename pairs kernels
whose own name changed, e.g. --rename 'pass_interval_kernel<5>=pass_kernel<5>'.
  identical : same instruction text, same three resource values
  mnemonics : same mnemonics in the same order, same resource values; operands differ (e.g. kernel-argument offsets)
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES = ("num_vgpr", "numbered_sgpr", "private_seg_size")


def emit(outdir, csrc):
    from mulut_amd import _native
    os.makedirs(outdir, exist_ok=True)
    flags = [f for f in _native.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    procs = [(s, subprocess.Popen([_native._hipcc()] + flags + ["--cuda-device-only", "-S", "-o", os.path.join(os.path.abspath(outdir), s[:-4] + ".s"), s],
                                  cwd=csrc, stderr=subprocess.DEVNULL)) for s in _native.SOURCES]
    bad = [s for s, p in procs if p.wait() != 0]
    if bad:
        sys.exit("failed to compile: %s" % " ".join(bad))


def cut(lines, name):
    """Lines of kernel `name` from its label to its .Lfunc_end (a kernel may hold several s_endpgm)."""
    out, on = [], False
    for line in lines:
        if line.startswith(name + ":"):
            on = True
        if on:
            out.append(line)
            if line.startswith(".Lfunc_end"):
                break
    return out


def normalise(body):
    labels, out = {}, []
    for line in body[1:]:
        line = line.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.startswith(".LBB")):
            continue
        out.append(re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), line))
    return out


def kernels(path):
    """{pairing key: (instruction lines, resource values)} of every kernel of an assembly file."""
    lines = open(path).read().splitlines()
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel (\S+)", l) for l in lines) if m]
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n") if names else []
    res = {}
    for l in lines:
        m = re.match(r"\s*\.set (\S+)\.(%s), (\d+)" % "|".join(RES), l)
        if m:
            res.setdefault(m.group(1), {})[m.group(2)] = int(m.group(3))
    out = {}
    for n, d in zip(names, plain):
        key = re.sub(r"^void ", "", d[:d.rindex("(")] if "(" in d else d).replace("mulut::", "")
        out[key] = (normalise(cut(lines, n)), tuple(res.get(n, {}).get(r) for r in RES))
    return out


def compare(old, new, renames, only):
    ren = dict(r.split("=", 1) for r in renames)
    files = lambda d: sorted(f[:-2] for f in os.listdir(d) if f.endswith(".s") and (not only or f[:-2] in only))
    a = {ren.get(k, k): (f, v) for f in files(old) for k, v in kernels(os.path.join(old, f + ".s")).items()}
    worst = 0
    for f in files(new):
        b = kernels(os.path.join(new, f + ".s"))
        print("== %s: %d kernels" % (f, len(b)))
        for k in sorted(b):
            if k not in a:
                print("  %-10s %s" % ("ONLY-NEW", k))
                worst = 2
                continue
            (fa, (ia, ra)), (ib, rb) = a.pop(k), b[k]
            if ia == ib and ra == rb:
                verdict = "identical"
            elif [x.split()[0] for x in ia] == [x.split()[0] for x in ib] and ra == rb:
                verdict, worst = "mnemonics", max(worst, 1)
            else:
                verdict, worst = "DIFFERENT", 2
            print("  %-10s %-60s instr %5d -> %5d  vgpr/sgpr/scratch %s -> %s%s" % (verdict, k, len(ia), len(ib), "/".join(map(str, ra)), "/".join(map(str, rb)),
                                                                                 "" if fa == f else "  (was in %s)" % fa))
    for k, (fa, _) in sorted(a.items()):
        print("  %-10s %s (%s)" % ("ONLY-OLD", k, fa))
        worst = 2
    return worst


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("emit")
    p.add_argument("outdir")
    p.add_argument("--csrc", default=os.path.join(ROOT, "mulut_amd", "csrc"))
    p = sub.add_parser("compare")
    p.add_argument("old")
    p.add_argument("new")
    p.add_argument("--rename", action="append", default=[])
    p.add_argument("--only", action="append", default=[])
    p = sub.add_parser("cut")
    p.add_argument("file")
    p.add_argument("name")
    args = ap.parse_args()
    if args.cmd == "emit":
        emit(args.outdir, args.csrc)
    elif args.cmd == "cut":
        print("\n".join(cut(open(args.file).read().splitlines(), args.name)))
    else:
        sys.exit(2 if compare(args.old, args.new, args.rename, args.only) == 2 else 0)
