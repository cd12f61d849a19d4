#!/usr/bin/env python3
"""Compare the device code of two builds of one translation unit, symbol by symbol.  CPU only.

    hipcc <HIPFLAGS of csrc/Makefile> --cuda-device-only -S -o before.s mgk_kernels.hip      (at the parent)
    hipcc <HIPFLAGS of csrc/Makefile> --cuda-device-only -S -o after.s  mgk_kernels.hip      (at the change)
    python tools/compare_device_asm.py before.s after.s

Prints one line per symbol that is in one file only, whose instructions differ, or whose kernel descriptor (.amdhsa_* directives: VGPR /
SGPR / AGPR counts, LDS and scratch size, ...) differs; prints nothing and exits 0 when the device code is the same.  Functions are matched
by name, so moving an instantiation point (which reorders the functions and renumbers their local labels) is no difference: the function
number in .LBB<function>_<block> labels is dropped before comparing, comments are stripped."""
import re
import sys


def parse(path):
    funcs, descs = {}, {}
    cur = body = kind = None
    kern = desc = None                 # the descriptor block lies inside its function, before the function's end label
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].rstrip()
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kern, desc = m.group(1), []
            continue
        if desc is not None:
            if re.match(r"\s*\.end_amdhsa_kernel", line):
                descs[kern] = desc
                desc = None
            elif line.strip():
                desc.append(" ".join(line.split()))
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur, body, kind = m.group(1), [], "func"
            continue
        if kind == "func":
            if re.match(r"\.Lfunc_end\d+:", line):
                funcs[cur] = body
                kind = None
                continue
            s = " ".join(line.split())
            if not s or s == cur + ":" or s.startswith(".p2align") or s.startswith(".globl") or s.startswith(".protected"):
                continue
            body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s))
    return funcs, descs


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (fa, da), (fb, db) = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for what, a, b in (("function", fa, fb), ("kernel descriptor", da, db)):
        for sym in sorted(set(a) | set(b)):
            if sym not in a or sym not in b:
                print(f"{what} only in {sys.argv[2] if sym in b else sys.argv[1]}: {sym}")
            elif a[sym] != b[sym]:
                at = next((i for i, (x, y) in enumerate(zip(a[sym], b[sym])) if x != y), min(len(a[sym]), len(b[sym])))
                print(f"{what} differs: {sym} (line {at} of {len(a[sym])} / {len(b[sym])})")
            else:
                continue
            bad += 1
    print(f"{len(fa)} / {len(fb)} functions, {len(da)} / {len(db)} kernel descriptors compared", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
