#!/usr/bin/env python3
"""Per-kernel device assembly of two trees' copies of a HIP source, side by side.

    tools/asm_diff.py node_persistent.hip gat_fused.hip --base ../parent --new .

For each named file of neuralgraphpde.jl_amd/csrc it compiles both trees' copies with the Makefile's flags for that file (CXXFLAGS
and EXTRA_<name>) plus --cuda-device-only -S -Rpass-analysis=kernel-resource-usage, splits the output per kernel symbol, drops
comments and directives, renames basic-block labels by their order, and prints per kernel: the instruction count, "identical" or the
number of lines changed (difflib opcodes: replaced, inserted and deleted lines, so a renamed register counts every line it is in), and
VGPR / AGPR / SGPR, spills, scratch bytes per lane, LDS and occupancy of both sides where the text differs (--all: always).
It compares text only; it needs the compiler, not a GPU.
Limits: the flags are read from `make -pnq` as plain `NAME =`, `:=` or `?=` assignments with `$(NAME)` references -- a flag added
with `+=`, a target-specific variable or a `${NAME}` would be missed; a kernel's body is found at the first line `<symbol>:`.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys

CSRC = os.path.join("neuralgraphpde.jl_amd", "csrc")
RES = [("VGPR", r"VGPRs: (\d+)"), ("AGPR", r"AGPRs: (\d+)"), ("SGPR", r"SGPRs: (\d+)"), ("spilled SGPR", r"SGPRs Spill: (\d+)"),
       ("spilled VGPR", r"VGPRs Spill: (\d+)"), ("scratch B/lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
       ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("LDS B", r"LDS Size \[bytes/block\]: (\d+)")]


def make_flags(tree, name):
    """CXXFLAGS and EXTRA_<name> as the Makefile expands them (its HIPCC too)."""
    db = subprocess.run(["make", "-C", os.path.join(tree, CSRC), "-pnq"], capture_output=True, text=True).stdout
    var = {m.group(1): m.group(2) for m in re.finditer(r"^(\w+) \??:?= *(.*)$", db, re.M)}
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: expand(var.get(m.group(1), "")), s)
    return expand(var["HIPCC"]), (expand(var["CXXFLAGS"]) + " " + expand(var.get("EXTRA_" + name, ""))).split()


def compile_asm(tree, src):
    hipcc, flags = make_flags(tree, src[:-4])
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", "-", src]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    return r.stdout, r.stderr


def kernels(asm, remarks):
    """{symbol: (instruction lines, resources)} in the order of the file."""
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    out = {}
    for sym in names:
        body = asm[asm.index("\n%s:" % sym):]
        body = body[:body.index(".Lfunc_end")].split("\n")[2:]
        labels, lines = {}, []
        for ln in body:
            ln = ln.split(";")[0].strip()
            m = re.match(r"(\.LBB\w+):$", ln)
            if m:
                labels[m.group(1)] = "L%d" % len(labels)
            elif ln and not ln.startswith("."):
                lines.append(ln)
        lines = [re.sub(r"\.LBB\w+", lambda m: labels.get(m.group(0), m.group(0)), ln) for ln in lines]
        m = re.search(r"Function Name: %s\b(.*?)LDS Size[^\n]*" % re.escape(sym), remarks, re.S)
        res = {k: int(re.search(p, m.group(0)).group(1)) for k, p in RES} if m else {}
        out[sym] = (lines, res)
    return out


def demangle(syms):
    r = subprocess.run(["c++filt", "-p"], input="\n".join(syms), capture_output=True, text=True)
    short = [re.sub(r"(?:ngpde|\(anonymous namespace\))::", "", s) for s in r.stdout.split("\n")] if r.returncode == 0 else syms
    return dict(zip(syms, short))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src", nargs="+", help="file names inside neuralgraphpde.jl_amd/csrc")
    ap.add_argument("--base", required=True, help="root of the tree to compare against")
    ap.add_argument("--new", required=True, help="root of the tree under test")
    ap.add_argument("--all", action="store_true", help="print the resources of identical kernels too")
    a = ap.parse_args()
    for src in a.src:
        kb, kn = kernels(*compile_asm(a.base, src)), kernels(*compile_asm(a.new, src))
        names = demangle(list(kn))
        same = 0
        print("%s\n  %-58s %12s   against the base" % (src, "kernel", "instructions"))
        for sym, (ln, rn) in kn.items():
            if sym not in kb:
                print("  %-58s %12d   new kernel" % (names[sym], len(ln)))
                continue
            lb, rb = kb[sym]
            changed = sum(max(i2 - i1, j2 - j1) for op, i1, i2, j1, j2 in
                          difflib.SequenceMatcher(None, lb, ln, autojunk=False).get_opcodes() if op != "equal")
            same += changed == 0
            verdict = "identical" if changed == 0 else "differs (%d -> %d, %d lines changed)" % (len(lb), len(ln), changed)
            print("  %-58s %12d   %s" % (names[sym], len(ln), verdict))
            if changed or a.all or rb != rn:
                for side, r in (("base", rb), ("new", rn)):
                    print("  %58s %s" % (side, "  ".join("%s %d" % (k, r[k]) for k, _ in RES if k in r)))
        gone = [s for s in kb if s not in kn]
        print("  %d kernels: %d identical, %d differ%s" % (len(kn), same, len(kn) - same, "; missing: " + " ".join(gone) if gone else ""))


if __name__ == "__main__":
    main()
