#!/usr/bin/env python3
"""What the line tail kernel replaces, from two rocprofv3 --kernel-trace runs of the SAME solve (csv output): one with line_tail = 1, one made
launch by launch (line_tail = 0, or a build of the parent commit).  The two dispatch sequences are equal except that each tail kernel stands
for a run of R launches, R = (dispatches without - dispatches with) / tail kernels + 1.  Prints, per tail kernel: its duration, the summed
durations of the R launches it replaces and the time from the start of the first to the end of the last of them (which includes the gaps
between launches); then medians, and the replaced launches by kernel name.
usage: line_tail_trace.py DIR_WITH DIR_WITHOUT [--out FILE]"""
import csv
import glob
import json
import os
import statistics
import sys


def load(d):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert f, "no kernel trace under " + d
    rows = []
    for r in csv.DictReader(open(f[-1])):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def short(name):
    return name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0][:60]


on, off = load(sys.argv[1]), load(sys.argv[2])
tails = [k for k, r in enumerate(on) if "k_tail_line" in r[2]]
K = len(tails)
assert K, "no tail kernel in " + sys.argv[1]
extra = len(off) - len(on)
assert extra % K == 0, (len(off), len(on), K)
R = extra // K + 1
j, per, names, mismatches = 0, [], {}, 0
for s, e, name in on:
    if "k_tail_line" in name:
        run = off[j:j + R]
        per.append(((e - s) / 1e3, sum(b - a for a, b, _ in run) / 1e3, (run[-1][1] - run[0][0]) / 1e3))
        for a, b, nm in run:
            q = names.setdefault(short(nm), [0, 0.0])
            q[0] += 1
            q[1] += (b - a) / 1e3
        j += R
    else:
        mismatches += off[j][2] != name
        j += 1
print(f"{len(on)} dispatches with the tail, {len(off)} without, {K} tail kernels: each stands for {R} launches; {mismatches} names out of step")
tail_us = statistics.median(p[0] for p in per)
sum_us = statistics.median(p[1] for p in per)
span_us = statistics.median(p[2] for p in per)
print(f"median over the {K} cycles: tail kernel {tail_us:.1f} us; the {R} launches it replaces: {sum_us:.1f} us of kernel time, {span_us:.1f} us from first start to last end")
for nm, (cnt, us) in sorted(names.items(), key=lambda kv: -kv[1][1]):
    print(f"  {cnt // K:3d} x {nm:60s} {us / K:8.1f} us per cycle")
if len(sys.argv) > 4 and sys.argv[3] == "--out":
    with open(sys.argv[4], "a") as fo:
        fo.write(json.dumps({"with": sys.argv[1], "without": sys.argv[2], "dispatches_with": len(on), "dispatches_without": len(off), "tail_kernels": K,
                             "launches_replaced": R, "names_out_of_step": mismatches, "tail_us_median": tail_us, "replaced_kernel_us_median": sum_us,
                             "replaced_span_us_median": span_us, "per_cycle": per,
                             "replaced_by_kernel_per_cycle": {nm: [cnt / K, us / K] for nm, (cnt, us) in names.items()}}) + "\n")
