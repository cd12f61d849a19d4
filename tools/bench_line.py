"""The line-smoothed cycles (pc_type="yline", and "altline": y- and x-line sweeps in turn) against the point-Jacobi cycle and against
V-cycle-preconditioned GMRES over it, one GPU, time to rtol 1e-7 at Richardson scale 0.8.  Per case ONE process holds two or three solvers of the same configuration; the samples alternate
between them (drift of the machine hits all alike), after one warm-up of each (first launches, the graph recording, the basis allocation).
Reported per case: iterations, every sample of solve_seconds, and whether EVERY yline sample lies below EVERY sample of the others.

    python tools/bench_line.py --case 4097:1:30 [--samples 5] [--only yline|altline|xline|jacobi|gmres] [--chunk C] [--xchunk C] [--line-tail 1] [--out FILE]      (run one case per process)
    python tools/bench_line.py --kernels 4095,2047,1023 [--depths 8,16,32] [--xdepths 1,2,3] [--chunk C] [--xchunk C,C,..] [--uniform] [--reps 20] [--out FILE]

A case is npts:mesh[:restart]; with a restart length solve_gmres(restart) on a point-Jacobi solver is the third contender.  --only runs one
alone (one solve of it under a kernel trace).  --kernels times the two passes of a y sweep and of an x sweep alone (from a guess, in place) on
an n x n level with random row tables for every built prefetch depth (y: rows, x: tiles of 16 columns): the measurement behind the default
depths and the x : y pass ratio.  --chunk C (line_chunk): the yline and altline solvers make their y sweeps in chunks of C
rows; with --kernels the four passes of a chunked y sweep are timed as well (under "chunk_<C>": per pass and per sweep the time of 10 launches back to back and one synchronise, over 10; the plain sweep is timed the
same way under "depth_<D>"/"sweep", beside the plain passes).  --xchunk C (xline_chunk): the xline and altline solvers make
their x sweeps in chunks of C columns; with --kernels (a list of C is taken) the four passes of a chunked x sweep are timed in the same way under
"xchunk_<C>", and the plain x sweep of every depth back to back under "xdepth_<D>"/"sweep".  --line-tail 1 (line_tail): the
line solvers run the coarse levels that fit in LDS as one kernel per cycle; the row then carries line_tail and every solver's tail_level.  --uniform: the x tables in the stride-0 form of the
uniform mesh (one row for every grid row)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from multigrid_petsc_amd.solver import Solver  # noqa: E402

RTOL = 1e-7
SCALE = 0.8
INNER = 10          # --chunk with --kernels: launches per timed sample (a chunked pass is tens of microseconds: one launch + sync would measure the sync)


def run(npts, mesh, restart, samples, only, chunk=0, xchunk=0, line_tail=0):
    levels = (npts - 1).bit_length() - 1
    kinds = [only] if only else ["yline", "altline", "jacobi"] + (["gmres"] if restart else [])
    tail = lambda k: dict(line_tail=1) if line_tail and k in ("yline", "xline", "altline") else {}
    S = {k: Solver(2, npts, levels, v=(3, 3), scale=SCALE, maxiter=2000, rtol=RTOL, mesh=mesh, pc_type="jacobi" if k == "gmres" else k,
                   line_chunk=chunk if k in ("yline", "altline") else 0, xline_chunk=xchunk if k in ("xline", "altline") else 0, **tail(k))
         for k in kinds}
    call = {k: (lambda s: s.solve()) for k in ("yline", "altline", "xline", "jacobi")}
    call["gmres"] = lambda s: s.solve_gmres(restart)
    secs, its = {k: [] for k in kinds}, {}
    for k, s in S.items():
        s.set_rhs_problem()
        call[k](s)                                                        # warm-up
    for _ in range(samples):
        for k, s in S.items():
            s.reset()
            its[k] = call[k](s)
            secs[k].append(s.solve_seconds)
    row = {"npts": npts, "levels": levels, "mesh": mesh, "scale": SCALE, "restart": restart, "rtol": RTOL, "samples": samples, "line_chunk": chunk, "xline_chunk": xchunk,
           "line_tail": line_tail}
    for k, s in S.items():
        rn = s.rnorm
        row[k] = {"iterations": its[k], "converged": bool(rn[-1] <= RTOL * s.bnorm), "relative_residual": float(rn[-1] / rn[0]),
                  "seconds": secs[k], "seconds_median": statistics.median(secs[k])}
        if line_tail:
            row[k]["tail_level"] = s.tail_level
        s.close()
    for k in kinds:
        if k != "yline" and "yline" in kinds:
            row[k + "_over_yline"] = row[k]["seconds_median"] / row["yline"]["seconds_median"]
            row["every_yline_sample_below_every_%s_sample" % k] = max(secs["yline"]) < min(secs[k])
    return row


def kernels(sizes, depths, xdepths, reps, chunk=0, xchunks=(), uniform=False):
    """microseconds of one forward and one backward pass (from a guess, in place) per size and prefetch depth, median of `reps`: the y passes
    under "depth_<rows>", the x passes under "xdepth_<tiles>" """
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import line_reference as LR
    import xline_reference as XR
    from row_tables import _rt_tables
    from multigrid_petsc_amd.mgk import Mgk
    m = Mgk(0)
    L = m.L
    rows = []
    for n in sizes:
        ct = _rt_tables(np.random.default_rng(n + 1), n)[0]           # (the time of a pass does not depend on the values)
        if uniform:
            ct = np.tile(ct[1], (n, 1))
        l, g, q = LR.tables(ct)
        geo = m.geom(2, n)
        rng = np.random.default_rng(n)
        b, u = m.to_field(geo, rng.uniform(-1, 1, n * n)), m.to_field(geo, rng.uniform(-1, 1, n * n))
        z = m.field(geo)
        t = [m.upload(x) for x in (ct, l, g, q)]
        gs = 0 if uniform else (n + 15) // 16 * 16
        xg = np.zeros((1 if uniform else n, (n + 15) // 16 * 16))
        xg[:, :n] = XR.table(ct[:1] if uniform else ct, n)
        t.append(m.upload(xg.ravel()))
        G = C.byref(geo)
        row = {"n": n, "reps": reps, "uniform": uniform}
        for d in depths:
            L.mgk_set_tuning(-1, d)
            us = {"forward": [], "backward": []}
            for r in range(reps + 2):
                m.sync()
                t0 = time.perf_counter()
                m._chk(L.mgk_line_forward_f64(m.ctx, G, t[0], t[1], t[2], b, u, z, None))
                m.sync()
                t1 = time.perf_counter()
                m._chk(L.mgk_line_backward_f64(m.ctx, G, t[3], 1e-3, z, u, u, None))
                m.sync()
                t2 = time.perf_counter()
                if r >= 2:
                    us["forward"].append(1e6 * (t1 - t0))
                    us["backward"].append(1e6 * (t2 - t1))
            row["depth_%d" % d] = {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in us.items()}
            if chunk >= 2:                                            # the plain sweep timed as the chunked one below: back to back
                sw = []
                for r in range(reps + 2):
                    m.sync()
                    t0 = time.perf_counter()
                    for _ in range(INNER):
                        m._chk(L.mgk_line_forward_f64(m.ctx, G, t[0], t[1], t[2], b, u, z, None))
                        m._chk(L.mgk_line_backward_f64(m.ctx, G, t[3], 1e-3, z, u, u, None))
                    m.sync()
                    if r >= 2:
                        sw.append(1e6 * (time.perf_counter() - t0) / INNER)
                row["depth_%d" % d]["sweep"] = {"median_us": statistics.median(sw), "min_us": min(sw)}
        for d in xdepths:
            L.mgk_set_tuning(-1, d)
            us = {"forward": [], "backward": []}
            for r in range(reps + 2):
                m.sync()
                t0 = time.perf_counter()
                m._chk(L.mgk_xline_forward_f64(m.ctx, G, t[0], t[4], gs, b, u, z, None))
                m.sync()
                t1 = time.perf_counter()
                m._chk(L.mgk_xline_backward_f64(m.ctx, G, t[0], t[4], gs, 1e-3, z, u, u, None))
                m.sync()
                t2 = time.perf_counter()
                if r >= 2:
                    us["forward"].append(1e6 * (t1 - t0))
                    us["backward"].append(1e6 * (t2 - t1))
            row["xdepth_%d" % d] = {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in us.items()}
            if xchunks:                                               # the plain x sweep timed as the chunked one below: back to back
                sw = []
                for r in range(reps + 2):
                    m.sync()
                    t0 = time.perf_counter()
                    for _ in range(INNER):
                        m._chk(L.mgk_xline_forward_f64(m.ctx, G, t[0], t[4], gs, b, u, z, None))
                        m._chk(L.mgk_xline_backward_f64(m.ctx, G, t[0], t[4], gs, 1e-3, z, u, u, None))
                    m.sync()
                    if r >= 2:
                        sw.append(1e6 * (time.perf_counter() - t0) / INNER)
                row["xdepth_%d" % d]["sweep"] = {"median_us": statistics.median(sw), "min_us": min(sw)}
        L.mgk_set_tuning(-1, -1)
        if chunk >= 2:
            import chunkline_reference as CR
            tab = CR.tables(ct, chunk)
            ch = {k: m.upload(tab[k] if tab[k].size else np.zeros(1)) for k in ("l", "g", "q", "v", "w", "L", "G", "Q")}
            calls = (("forward", lambda: L.mgk_line_chunk_forward_f64(m.ctx, G, chunk, t[0], ch["l"], ch["g"], b, u, z, None)),
                     ("backward", lambda: L.mgk_line_chunk_backward_f64(m.ctx, G, chunk, ch["q"], z, None)),
                     ("reduce", lambda: L.mgk_line_chunk_reduce_f64(m.ctx, G, chunk, t[0], ch["L"], ch["G"], ch["Q"], z, None)),
                     ("correct", lambda: L.mgk_line_chunk_correct_f64(m.ctx, G, chunk, ch["v"], ch["w"], 1e-3, z, u, u, None)))
            us = {k: [] for k, _ in calls}
            us["sweep"] = []                                          # the four launches back to back, one synchronise
            for r in range(reps + 2):
                for k, f in calls:                                    # a pass: INNER launches back to back, one synchronise, per launch
                    m.sync()
                    t0 = time.perf_counter()
                    for _ in range(INNER):
                        m._chk(f())
                    m.sync()
                    if r >= 2:
                        us[k].append(1e6 * (time.perf_counter() - t0) / INNER)
                t0 = time.perf_counter()
                for _ in range(INNER):
                    for k, f in calls:
                        m._chk(f())
                m.sync()
                if r >= 2:
                    us["sweep"].append(1e6 * (time.perf_counter() - t0) / INNER)
            row["chunk_%d" % chunk] = {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in us.items()}
            t += list(ch.values())
        for xc in xchunks:
            import xchunkline_reference as XC
            K, n16 = n // xc, (n + 15) // 16 * 16
            # the time of a pass does not depend on the values: the tables of 16 rows (uniform: of the one row there is), repeated down the grid
            tab = XC.tables(ct[:1] if uniform else ct[:16], xc, n)
            rep = 1 if uniform else (n + 15) // 16

            def wide(a):
                o = np.zeros((a.shape[0] * rep, n16))
                o[:, :n] = np.tile(a, (rep, 1))
                return o[:1 if uniform else n].ravel()

            def tall(a):                                              # separator-major
                if uniform:
                    return a[0] if K else np.zeros(1)
                o = np.zeros((max(K, 1), n16))
                o[:K, :n] = np.tile(a, (rep, 1))[:n].T
                return o.ravel()

            ch = {k: m.upload(wide(tab[k])) for k in ("g", "v", "w")}
            ch.update({k: m.upload(tall(tab[k])) for k in ("SL", "SG", "SQ")})
            ch["sep"] = m.upload(np.zeros(4 * max(K, 1) * n16))
            sst = 0 if uniform else n16
            calls = (("forward", lambda: L.mgk_xline_chunk_forward_f64(m.ctx, G, xc, t[0], ch["g"], gs, b, u, z, ch["sep"], None)),
                     ("backward", lambda: L.mgk_xline_chunk_backward_f64(m.ctx, G, xc, t[0], ch["g"], gs, z, ch["sep"], None)),
                     ("reduce", lambda: L.mgk_xline_chunk_reduce_f64(m.ctx, G, xc, t[0], ch["SL"], ch["SG"], ch["SQ"], sst, ch["sep"], None)),
                     ("correct", lambda: L.mgk_xline_chunk_correct_f64(m.ctx, G, xc, ch["v"], ch["w"], gs, 1e-3, z, ch["sep"], u, u, None)))
            us = {k: [] for k, _ in calls}
            us["sweep"] = []                                          # the four launches back to back, one synchronise
            for r in range(reps + 2):
                for k, f in calls:                                    # a pass: INNER launches back to back, one synchronise, per launch
                    m.sync()
                    t0 = time.perf_counter()
                    for _ in range(INNER):
                        m._chk(f())
                    m.sync()
                    if r >= 2:
                        us[k].append(1e6 * (time.perf_counter() - t0) / INNER)
                t0 = time.perf_counter()
                for _ in range(INNER):
                    for k, f in calls:
                        m._chk(f())
                m.sync()
                if r >= 2:
                    us["sweep"].append(1e6 * (time.perf_counter() - t0) / INNER)
            row["xchunk_%d" % xc] = {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in us.items()}
            for p in ch.values():
                m.free(p)
        for p in [b, u, z] + t:
            m.free(p)
        rows.append(row)
    m.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="npts:mesh[:restart]")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["yline", "altline", "xline", "jacobi", "gmres"])
    ap.add_argument("--kernels", default=None, help="level sizes n (n + 1 a power of two), comma separated")
    ap.add_argument("--depths", default="8,16,32")
    ap.add_argument("--xdepths", default="1,2,3")
    ap.add_argument("--chunk", type=int, default=0, help="line_chunk of the yline / altline solvers; with --kernels: time the four chunked passes too")
    ap.add_argument("--xchunk", default="0", help="xline_chunk of the xline / altline solvers; with --kernels: a list, time the four chunked x passes of each")
    ap.add_argument("--line-tail", type=int, default=0, choices=[0, 1],
                    help="--case: 1 = the line solvers run their LDS-resident coarse levels in one launch (mg_config.line_tail, DESIGN.md section 8j)")
    ap.add_argument("--uniform", action="store_true", help="--kernels: the x tables in the stride-0 form of the uniform mesh")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernels:
        rows = kernels([int(x) for x in a.kernels.split(",")], [int(x) for x in a.depths.split(",") if x], [int(x) for x in a.xdepths.split(",") if x], a.reps, a.chunk,
                       [int(x) for x in a.xchunk.split(",") if int(x) > 0], a.uniform)
    elif a.case:
        if "," in a.xchunk:
            ap.error("--case takes one --xchunk value (a list goes with --kernels)")
        f = a.case.split(":")
        rows = [run(int(f[0]), int(f[1]), int(f[2]) if len(f) > 2 else 0, a.samples, a.only, a.chunk, int(a.xchunk), a.line_tail)]
    else:
        ap.error("give --case or --kernels")
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as fo:
            for r in rows:
                fo.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
