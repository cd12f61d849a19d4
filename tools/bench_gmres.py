"""V-cycle-preconditioned GMRES against the plain V-cycle iteration, one GPU, time to rtol 1e-7.  Per case ONE process holds two solvers of
the same configuration; the samples alternate between solve() and solve_gmres(restart) (drift of the machine hits both alike), after one
warm-up of each (first launches, the graph recording, the basis allocation).  Reported per case: iterations (V-cycles / Arnoldi steps and
applications of the cycle), every sample of solve_seconds, and whether EVERY sample of one lies below EVERY sample of the other.

    python tools/bench_gmres.py [--cases 2:4097:0:0.8:30,...] [--samples 5] [--only solve|gmres] [--out FILE]

A case is dim:npts:mesh:scale:restart.  Default: 4097^2 on meshes 0, 1, 2 at the bench's scale (0.8), 4097^2 mesh 0 at scale 1, 511^3
(npts 513) at 6/7 and at 1, restart 30 and 8.  --only runs one of the two alone (one solve of it under a kernel trace).  A plain iteration
that has not converged within its cap (scale 1: undamped Jacobi is not a smoother) is reported with converged = false."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multigrid_petsc_amd.solver import Solver  # noqa: E402

DEFAULT = "2:4097:0:0.8:30,2:4097:1:0.8:30,2:4097:2:0.8:30,2:4097:0:1.0:30,3:513:0:0.857142857142857:30,3:513:0:0.857142857142857:8,3:513:0:1.0:30,3:513:0:1.0:8"
RTOL = 1e-7


def run(dim, npts, mesh, scale, restart, samples, only):
    levels = (npts - 1).bit_length() - 1
    maxiter = 2000 if scale < 1.0 else 300
    kinds = [only] if only else ["solve", "gmres"]
    S = {k: Solver(dim, npts, levels, v=(3, 3), scale=scale, maxiter=maxiter, rtol=RTOL, mesh=mesh) for k in kinds}
    call = {"solve": lambda s: s.solve(), "gmres": lambda s: s.solve_gmres(restart)}
    secs, its = {k: [] for k in kinds}, {}
    for k, s in S.items():
        s.set_rhs_problem()
        call[k](s)                                                        # warm-up
    for _ in range(samples):
        for k, s in S.items():
            s.reset()
            its[k] = call[k](s)
            secs[k].append(s.solve_seconds)
    row = {"dim": dim, "npts": npts, "levels": levels, "mesh": mesh, "scale": scale, "restart": restart, "rtol": RTOL, "samples": samples}
    for k, s in S.items():
        rn = s.rnorm
        row[k] = {"iterations": its[k], "converged": bool(rn[-1] <= RTOL * s.bnorm), "relative_residual": float(rn[-1] / rn[0]),
                  "seconds": secs[k], "seconds_median": statistics.median(secs[k])}
        if k == "gmres":
            row[k]["cycle_applications"] = its[k] + -(-its[k] // restart)
        s.close()
    if len(kinds) == 2:
        row["gmres_over_solve"] = row["gmres"]["seconds_median"] / row["solve"]["seconds_median"]
        row["every_gmres_sample_below_every_solve_sample"] = max(secs["gmres"]) < min(secs["solve"])
        row["every_solve_sample_below_every_gmres_sample"] = max(secs["solve"]) < min(secs["gmres"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT, help="dim:npts:mesh:scale:restart, comma separated (all levels)")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["solve", "gmres"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for spec in a.cases.split(","):
        f = spec.split(":")
        r = run(int(f[0]), int(f[1]), int(f[2]), float(f[3]), int(f[4]), a.samples, a.only)
        print(json.dumps(r), flush=True)
        rows.append(r)
        if a.out:
            with open(a.out, "w") as fo:
                for q in rows:
                    fo.write(json.dumps(q) + "\n")


if __name__ == "__main__":
    main()
