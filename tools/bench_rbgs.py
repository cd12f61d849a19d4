"""Red-black Gauss-Seidel (pc_type="rbgs") against the cycles the project already has, one GPU.  One process per case: the driver mode starts a
child per case under a time limit of its own and stops at the first child that fails.

    python tools/bench_rbgs.py --kernels 4095 [--reps 20] [--out FILE]              the passes alone on an n x n level
    python tools/bench_rbgs.py --case 4097:1 [--samples 5] [--package DIR] [--out FILE]   solves to rtol 1e-7
    python tools/bench_rbgs.py --suite kernels|solves|parent [--package DIR] [--out FILE] [--limit SECONDS]   every case of the write-up, a child each

--kernels: microseconds of one launch and TB/s of the ALGORITHMIC bytes (24 / 16 / 25 B per unknown: plain / zero guess / with prolongation)
of mgk_rbgs_2d_f64 and mgk_prolong_rbgs_2d_f64 with nsweeps 1 and 2, on constants and on row tables, and beside them, as the yardstick of the
same build, mgk_jacobi3_2d_f64 / _zero_f64 / mgk_prolong_jacobi3_2d_f64.  Random fields, not zeros.  A sample is INNER launches back to back
between two buffers (every launch reads what the one before wrote, as in a cycle) and one synchronise, per launch; median and minimum of
--reps samples after two warm-ups.

--case npts:mesh: point Jacobi V(3,3) at scale 0.8 (the default path), RB-GS V(1,1) and V(2,2) at scale 1 (v1 = 3 on the 1 x 1 level in
every configuration), and on meshes 1 / 2 altline with both chunks 128; the samples alternate between the solvers after one warm-up each.
--package DIR imports multigrid_petsc_amd from DIR instead (a build of another commit: its own libraries beside its Python files) and runs
the point-Jacobi configuration alone: the cross-check that nothing existing moved."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-7
INNER = 10
KERNEL_SIZES = (4095, 2047, 1023, 255)
SOLVE_CASES = [(npts, mesh) for npts in (1025, 4097, 16385) for mesh in (0, 1, 2)]


def kernels(n, reps):
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from row_tables import _rt_tables
    from multigrid_petsc_amd.mgk import Mgk
    m = Mgk(0)
    L = m.L
    nc = (n - 1) // 2
    gf, gc = m.geom(2, n), m.geom(2, nc)
    GF, GC = C.byref(gf), C.byref(gc)
    rng = np.random.default_rng(n)
    b, u, w = (m.to_field(gf, rng.uniform(-1, 1, n * n)) for _ in range(3))
    uc = m.to_field(gc, rng.uniform(-1, 1, nc * nc))
    ct, dt = _rt_tables(np.random.default_rng(n + 1), n)               # (the time of a pass does not depend on the values)
    dct, ddt = m.upload(ct), m.upload(dt)
    q = float((n + 1) ** 2)
    coef, dinv, scale = m.coef([q, q, -4.0 * q, q, q]), -0.25 / q, 0.8
    row = {"n": n, "reps": reps, "inner": INNER, "unknowns": n * n}
    for tab in (False, True):
        k, d, T, D = (None, 1.0, dct, ddt) if tab else (coef, dinv, None, None)
        calls = {}
        for ns in (1, 2):
            calls[f"rbgs{ns}_plain"] = (24, lambda s, o, ns=ns: L.mgk_rbgs_2d_f64(m.ctx, GF, k, d, scale, T, D, ns, b, s, o, None))
            calls[f"rbgs{ns}_zero"] = (16, lambda s, o, ns=ns: L.mgk_rbgs_2d_f64(m.ctx, GF, k, d, scale, T, D, ns, b, None, o, None))
            calls[f"rbgs{ns}_prolong"] = (25, lambda s, o, ns=ns: L.mgk_prolong_rbgs_2d_f64(m.ctx, GF, GC, k, d, scale, T, D, ns, b, uc, s, o, None))
        calls["jacobi3_plain"] = (24, lambda s, o: L.mgk_jacobi3_2d_f64(m.ctx, GF, k, d, scale, T, D, b, s, o, None))
        calls["jacobi3_zero"] = (16, lambda s, o: L.mgk_jacobi3_2d_zero_f64(m.ctx, GF, k, d, scale, T, D, b, o, None))
        calls["jacobi3_prolong"] = (25, lambda s, o: L.mgk_prolong_jacobi3_2d_f64(m.ctx, GF, GC, k, d, scale, T, D, b, uc, s, o, None))
        out = {}
        for name, (bytes_per, f) in calls.items():
            us = []
            for r in range(reps + 2):
                m._chk(L.mgk_memset0(m.ctx, w, 8 * gf.total, None))     # (a contraction at scale 0.8 from bounded data: nothing overflows)
                m.sync()
                t0 = time.perf_counter()
                for i in range(INNER):
                    m._chk(f(u, w) if i % 2 == 0 else f(w, u))
                m.sync()
                if r >= 2:
                    us.append(1e6 * (time.perf_counter() - t0) / INNER)
            med = statistics.median(us)
            out[name] = {"median_us": med, "min_us": min(us), "algorithmic_bytes_per_unknown": bytes_per, "tb_per_s": bytes_per * n * n / med * 1e-6}
        row["row_tables" if tab else "constants"] = out
    for p in (b, u, w, uc, dct, ddt):
        m.free(p)
    m.close()
    return row


def solves(npts, mesh, samples, package):
    sys.path.insert(0, package or ROOT)
    from multigrid_petsc_amd.solver import Solver
    levels = (npts - 1).bit_length() - 1
    cfgs = {"jacobi_v33_s0.8": dict(v=(3, 3), scale=0.8, pc_type="jacobi")}
    if not package:
        cfgs["rbgs_v11_s1"] = dict(v=(1, 3), scale=1.0, pc_type="rbgs")
        cfgs["rbgs_v22_s1"] = dict(v=(2, 3), scale=1.0, pc_type="rbgs")
        if mesh:
            cfgs["altline_v33_s0.8_chunks128"] = dict(v=(3, 3), scale=0.8, pc_type="altline", line_chunk=128, xline_chunk=128)
    S = {k: Solver(2, npts, levels, maxiter=400, rtol=RTOL, mesh=mesh, **kw) for k, kw in cfgs.items()}
    secs, its = {k: [] for k in S}, {}
    for k, s in S.items():
        s.set_rhs_problem()
        s.solve()                                                        # warm-up: first launches, the graph recording
    for _ in range(samples):
        for k, s in S.items():
            s.reset()
            its[k] = s.solve()
            secs[k].append(s.solve_seconds)
    row = {"npts": npts, "levels": levels, "mesh": mesh, "rtol": RTOL, "samples": samples, "package": package or "this build"}
    for k, s in S.items():
        rn = s.rnorm
        row[k] = {"iterations": its[k], "converged": bool(rn[-1] <= RTOL * s.bnorm), "relative_residual": float(rn[-1] / rn[0]),
                  "seconds": secs[k], "seconds_median": statistics.median(secs[k]), "ms_per_cycle": 1e3 * statistics.median(secs[k]) / max(its[k], 1)}
        s.close()
    return row


def suite(which, package, out, limit):
    """every case in a child process of its own, each under its own time limit; the first failure ends the suite"""
    me = [sys.executable, os.path.abspath(__file__)]
    if which == "kernels":
        cmds = [me + ["--kernels", str(n)] for n in KERNEL_SIZES]
    else:
        cmds = [me + ["--case", f"{npts}:{mesh}"] + (["--package", package] if which == "parent" else []) for npts, mesh in SOLVE_CASES]
    for cmd in cmds:
        p = subprocess.run(cmd + (["--out", out] if out else []), timeout=limit)
        if p.returncode != 0:
            print(f"bench_rbgs: {' '.join(cmd[2:])} ended with {p.returncode}: stopping", file=sys.stderr)
            return p.returncode
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", type=int, default=None, help="level size n (n + 1 a power of two)")
    ap.add_argument("--case", default=None, help="npts:mesh")
    ap.add_argument("--suite", default=None, choices=["kernels", "solves", "parent"])
    ap.add_argument("--package", default=None, help="directory that holds another build's multigrid_petsc_amd package")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=float, default=240.0, help="--suite: seconds a child may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.suite:
        if a.suite == "parent" and not a.package:
            ap.error("--suite parent needs --package")
        sys.exit(suite(a.suite, a.package, a.out, a.limit))
    if a.kernels:
        row = kernels(a.kernels, a.reps)
    elif a.case:
        f = a.case.split(":")
        row = solves(int(f[0]), int(f[1]), a.samples, a.package)
    else:
        ap.error("give --kernels, --case or --suite")
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as fo:
            fo.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
