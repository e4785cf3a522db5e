#!/usr/bin/env python3
"""The device code of two trees' csrc/, kernel by kernel (the method of profiles/detector_driver_isa.txt).  No GPU needed.

    python tools/isa_compare.py PARENT_CSRC TREE_CSRC [--renamed PREFIX ...] [--files A.hip B.hip ...]

Every *.hip of either directory that holds a __global__ function is compiled with build.py's flags plus
--cuda-device-only -S and one -cuid; each .s is split per function, from its label to its .Lfunc_end (which takes in
the .amdhsa_kernel descriptor); comment text, blank lines and .loc / .file / .cfi / .p2align / .section lines are dropped
and the rest compared line by line, whole lines only.  Functions are matched by mangled name across ALL files, so a kernel
that moved to another source is found (the ordinal of the function in its file, which local labels carry, is taken out of
them); one whose argument list changed (--renamed: a prefix of its mangled name) is matched by that prefix, its own name
replaced before the comparison.  Every function that is not identical is printed as a diff."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_mix

DROP = re.compile(r"^\s*\.(loc|file|cfi\w*|p2align|section)\b")
# local labels carry the function's ordinal in its file (.LBB4_1, .Lfunc_end4): it changes when a kernel moves
LOCAL = re.compile(r"\.L(BB|func_end|func_begin)\d+_?")


def assemble(src):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + isa_mix.FLAGS + ["-fPIC", "-cuid=icelk", os.path.abspath(src), "-o", out],
                          stderr=subprocess.DEVNULL, cwd="/tmp")
    return out


def functions(asm):
    """{mangled name: [lines]} of one .s"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", asm, flags=re.M | re.S):
        lines = []
        for line in m.group(0).split("\n"):
            line = line.split(";")[0].rstrip()
            if line.strip() and not DROP.match(line):
                lines.append(LOCAL.sub(r".L\1_", line))
        out[m.group(1)] = lines
    return out


def tree(csrc, only):
    """{name: (file, lines)} of every kernel under csrc"""
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and "__global__" in open(os.path.join(csrc, f)).read())
    files = [f for f in files if not only or f in only]
    with ThreadPoolExecutor(max_workers=8) as ex:
        asms = list(ex.map(lambda f: assemble(os.path.join(csrc, f)), files))
    out = {}
    for f, path in zip(files, asms):
        for name, lines in functions(open(path).read()).items():
            out[name] = (f, lines)
        os.unlink(path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("--renamed", action="append", default=[])
    ap.add_argument("--files", nargs="*", default=[], help="only these sources (default: all)")
    args = ap.parse_args()
    P, T = tree(args.parent, args.files), tree(args.tree, args.files)
    pairs = [(n, n) for n in sorted(P) if n in T]
    for prefix in args.renamed:
        a = [n for n in P if n.startswith(prefix) and n not in T]
        b = [n for n in T if n.startswith(prefix) and n not in P]
        if len(a) == 1 and len(b) == 1:
            pairs.append((a[0], b[0]))
    matched_p, matched_t = {a for a, _ in pairs}, {b for _, b in pairs}
    same = 0
    for a, b in pairs:
        fa, la = P[a]
        fb, lb = T[b]
        lb = [line.replace(b, a) for line in lb]
        where = fa if fa == fb else "%s -> %s" % (fa, fb)
        if la == lb:
            same += 1
            if fa != fb:
                print("moved, identical: %s (%s)" % (a, where))
            continue
        print("DIFFERS: %s (%s)%s" % (a, where, "" if a == b else "\n   renamed to %s" % b))
        for line in difflib.unified_diff(la, lb, "parent", "tree", lineterm="", n=2):
            print("      " + line)
    for n in sorted(set(P) - matched_p):
        print("ONLY IN PARENT: %s (%s)" % (n, P[n][0]))
    for n in sorted(set(T) - matched_t):
        print("ONLY IN TREE: %s (%s)" % (n, T[n][0]))
    print("%d functions in the parent, %d in the tree; %d compared, %d identical" % (len(P), len(T), len(pairs), same))


if __name__ == "__main__":
    main()
