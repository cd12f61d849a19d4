#!/usr/bin/env python3
"""Compare the device code of two builds, symbol by symbol.  CPU only.  Each side is one translation unit or several: the union of the
files of a side is compared, so a unit that was cut into several (or several merged into one) compares against what it was.

    hipcc <HIPFLAGS of csrc/Makefile> --cuda-device-only -S -o parent/<unit>.s <unit>.hip      (at the parent, per unit)
    hipcc <HIPFLAGS of csrc/Makefile> --cuda-device-only -S -o change/<unit>.s <unit>.hip      (at the change, per unit)
    python tools/compare_device_asm.py parent/mgk_line.s change/mgk_line.s
    python tools/compare_device_asm.py --before parent/mgk_kernels.s --after change/mgk_kernels.s change/mgk_tail.s

Prints one line per symbol that is on one side only, whose instructions differ, or whose kernel descriptor (.amdhsa_* directives: VGPR /
SGPR / AGPR counts, LDS and scratch size, ...) differs, and one line per symbol that occurs in MORE THAN ONE FILE of a side (a kernel
instantiated in two units); prints nothing and exits 0 when the device code is the same and every symbol has one home.  Functions are
matched by name, so moving an instantiation point (which reorders the functions and renumbers their local labels) is no difference: the
function number in .LBB<function>_<block> labels is dropped before comparing, comments are stripped."""
import argparse
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


def parse_side(paths):
    """Union of the files of one side; returns (functions, descriptors, number of symbols found in more than one file)."""
    funcs, descs, home, twice = {}, {}, {}, 0
    for path in paths:
        f, d = parse(path)
        for what, new, all_ in (("function", f, funcs), ("kernel descriptor", d, descs)):
            for sym in sorted(new):
                if sym in all_:
                    print(f"{what} in two files: {sym} ({home[what, sym]} and {path})")
                    twice += 1
                else:
                    all_[sym] = new[sym]
                    home[what, sym] = path
    return funcs, descs, twice


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pair", nargs="*", help="before.s after.s (one file a side)")
    ap.add_argument("--before", nargs="+", default=[], metavar="FILE.s")
    ap.add_argument("--after", nargs="+", default=[], metavar="FILE.s")
    args = ap.parse_args()
    if len(args.pair) == 2 and not args.before and not args.after:
        before, after = [args.pair[0]], [args.pair[1]]
    elif not args.pair and args.before and args.after:
        before, after = args.before, args.after
    else:
        ap.error("give either two files, or --before FILES --after FILES")
    (fa, da, ta), (fb, db, tb) = parse_side(before), parse_side(after)
    bad = ta + tb
    for what, a, b in (("function", fa, fb), ("kernel descriptor", da, db)):
        for sym in sorted(set(a) | set(b)):
            if sym not in a or sym not in b:
                print(f"{what} only {'after' if sym in b else 'before'}: {sym}")
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
