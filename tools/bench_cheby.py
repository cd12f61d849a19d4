"""Chebyshev smoothing on the fused cycle against its step-by-step path and against the Richardson cycle, one GPU.  Per size, three
configurations of the SAME process, alternating sample by sample: Chebyshev (0.2, 2.0) with the default fuse mask, Chebyshev with fuse
bit 15 off, Richardson + Jacobi (scale 0.8 in 2-D, 6/7 in 3-D).  ms per V(3,3) cycle: Solver.cycles after 2 warm-up cycles, as many cycles
per sample as make the timed window >= 0.2 s, the window closed by sync(); >= 5 samples each.  Then iterations and solve_seconds of
solve() to rtol 1e-7.  One JSON line per size.

    python tools/bench_cheby.py [--sizes 2:1025,2:2049,2:4097,3:129,3:257] [--samples 5] [--only cheby|cheby_off15|richardson] [--out FILE]

--only runs one configuration alone (a few cycles of it under a kernel trace, or the unfused path of another build of the library)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multigrid_petsc_amd.solver import Solver  # noqa: E402

DEFAULT_MASK = 63 | 0xFF00
EIG = (0.2, 2.0)


def make(kind, dim, npts, levels):
    if kind == "richardson":
        return Solver(dim, npts, levels, v=(3, 3), scale=6.0 / 7.0 if dim == 3 else 0.8, maxiter=1000, rtol=1e-7)
    fuse = -1 if kind == "cheby" else DEFAULT_MASK & ~32768
    return Solver(dim, npts, levels, v=(3, 3), ksp_type="chebyshev", eigenvalues=EIG, fuse=fuse, maxiter=1000, rtol=1e-7)


def window(s, k):
    s.sync()
    t0 = time.perf_counter()
    s.cycles(k)
    s.sync()
    return time.perf_counter() - t0


def run(dim, npts, kinds, samples, trace_cycles):
    levels = (npts - 1).bit_length() - 1
    S = {k: make(k, dim, npts, levels) for k in kinds}
    K, ms = {}, {k: [] for k in kinds}
    for k, s in S.items():
        s.set_rhs_problem()
        s.cycles(2)                                                      # warm-up: first launches, the graph recording
        if trace_cycles:
            K[k] = trace_cycles
            continue
        t = window(s, 4) / 4
        K[k] = max(4, int(0.2 / t) + 1)
    for _ in range(1 if trace_cycles else samples):
        for k, s in S.items():                                           # alternating: drift of the box hits every configuration alike
            ms[k].append(1e3 * window(s, K[k]) / K[k])
    row = {"dim": dim, "npts": npts, "levels": levels, "v": [3, 3], "eigenvalues": list(EIG), "samples": samples}
    for k, s in S.items():
        its, secs = [], []
        for _ in range(0 if trace_cycles else 3):
            s.reset()
            its.append(s.solve())
            secs.append(s.solve_seconds)
        row[k] = {"cycle_ms_median": statistics.median(ms[k]), "cycle_ms_min": min(ms[k]), "cycle_ms_max": max(ms[k]), "cycles_per_sample": K[k],
                  "solve_iters": its[-1] if its else None, "solve_seconds_median": statistics.median(secs) if secs else None}
        s.close()
    if "cheby" in row and "cheby_off15" in row:
        row["off15_over_cheby"] = row["cheby_off15"]["cycle_ms_median"] / row["cheby"]["cycle_ms_median"]
        # faster by more than the spread of the repetitions: the slowest fused sample against the quickest unfused one
        row["cheby_faster_than_off15_beyond_spread"] = row["cheby"]["cycle_ms_max"] < row["cheby_off15"]["cycle_ms_min"]
    if "cheby" in row and "richardson" in row:
        row["cheby_over_richardson"] = row["cheby"]["cycle_ms_median"] / row["richardson"]["cycle_ms_median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2:1025,2:2049,2:4097,3:129,3:257", help="dim:npts, comma separated (all levels)")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["cheby", "cheby_off15", "richardson"])
    ap.add_argument("--trace-cycles", type=int, default=0, help="no timing: just this many cycles per configuration (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    kinds = [a.only] if a.only else ["cheby", "cheby_off15", "richardson"]
    rows = []
    for spec in a.sizes.split(","):
        dim, npts = (int(x) for x in spec.split(":"))
        r = run(dim, npts, kinds, max(a.samples, 5), a.trace_cycles)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
