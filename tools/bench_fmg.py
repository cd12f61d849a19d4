"""Full multigrid on one GPU: time of FMG(1) against one V-cycle, time to rtol with and without FMG, and FMG(1)'s error against the
discretisation error (the error of the converged solution).  One JSON line per size.

    python tools/bench_fmg.py [--sizes 3:1025:10,3:513:9,2:4097:12] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multigrid_petsc_amd.solver import Solver  # noqa: E402


def _timed(fn, s):
    s.sync()
    t0 = time.perf_counter()
    fn()
    s.sync()
    return time.perf_counter() - t0


def run(dim, npts, levels, reps):
    scale = 6.0 / 7.0 if dim == 3 else 0.8
    s = Solver(dim, npts, levels, v=(3, 3), scale=scale, maxiter=1000, rtol=1e-7)
    s.set_rhs_problem()
    s.fmg(1)                                                             # warm-up: first launches, graph recording
    s.cycles(2)
    t_fmg = statistics.median(_timed(lambda: s.fmg(1), s) for _ in range(reps))
    efmg = s.error_norms()[0]
    k = 10
    s.reset()
    s.cycles(2)
    t_cyc = statistics.median(_timed(lambda: s.cycles(k), s) for _ in range(reps)) / k
    solve, solve_fmg = [], []
    for _ in range(reps):
        it_plain = s.solve()
        solve.append(s.solve_seconds)
        it_fmg = s.solve_fmg(1)
        solve_fmg.append(s.solve_seconds)
    s.close()
    d = Solver(dim, npts, levels, v=(3, 3), scale=scale, maxiter=1000, rtol=1e-12)
    d.set_rhs_problem()
    d.solve()
    edisc = d.error_norms()[0]
    d.close()
    return {"dim": dim, "npts": npts, "levels": levels, "v": [3, 3], "scale": scale,
            "fmg1_ms": 1e3 * t_fmg, "vcycle_ms": 1e3 * t_cyc, "fmg1_over_vcycle": t_fmg / t_cyc,
            "solve_ms": 1e3 * statistics.median(solve), "solve_iters": it_plain,
            "solve_fmg_ms": 1e3 * statistics.median(solve_fmg), "solve_fmg_iters": it_fmg,
            "err_fmg1": efmg, "err_disc": edisc, "err_ratio": efmg / edisc, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3:1025:10,3:513:9,2:4097:12", help="dim:npts:levels, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for spec in a.sizes.split(","):
        dim, npts, levels = (int(x) for x in spec.split(":"))
        r = run(dim, npts, levels, a.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
