"""The CG driver's two fused passes against the launches they replace, and whole solves: plain iteration, GMRES(30), CG.  One GPU.

    python tools/bench_cg.py passes [--shapes 2:4095,3:1023] [--samples 7] [--reps 5] [--out FILE]
    python tools/bench_cg.py solves [--cases 2:4097:0.8,...] [--samples 3] [--kinds solve,gmres,cg] [--out FILE]

passes: HIP events round `reps` back-to-back launches, after a warm-up of each version; the fused pass and the launches it replaces ALTERNATE
within one process, sample by sample (drift of the machine hits both alike); no call synchronises with the host (the fused passes are given
no host pointer, the replaced reductions run under mgk_defer_result).  Per shape one JSON line: every sample, median, min and max (the spread)
of both versions, the achieved bytes/s of the fused pass against its 32 B / 48 B per unknown, the STREAM triad measured in the same process
the way bench.py measures it, and whether EVERY fused sample lies below EVERY sample of the replaced launches.
  direction pass   mgk_cg_direction_apply_dot_f64      against  mgk_flat_aypx + mgk_apply_f64 + mgk_flat_dot        (24 + 16 + 16 B)
  update pass      mgk_cg_update_sumsq_f64             against  2 x mgk_flat_axpy + mgk_sumsq_f64                   (24 + 24 + 8 B)
solves: per case (dim:npts:scale, all levels, V(3,3), manufactured right-hand side, rtol 1e-7) one solver per kind in ONE process, the samples
alternating between the kinds after one warm-up of each; step counts and every sample of solve_seconds.  A plain iteration that has not
converged within its cap of 100 cycles is reported with converged = false."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

RTOL = 1e-7
COEF = {2: [-1.3, -0.7, 9.1, -1.1, -0.9], 3: [-0.6, -1.3, -0.7, 11.3, -1.1, -0.9, -0.8]}


def _stats(ms, reps):
    per = [v / reps for v in ms]
    return {"ms": per, "median_ms": statistics.median(per), "min_ms": min(per), "max_ms": max(per)}


def passes(dim, n, samples, reps):
    from multigrid_petsc_amd.mgk import Mgk, cg_sigs
    m = Mgk(0)
    L = m.L
    cg_sigs(L)
    g = m.geom(dim, n)
    N = n ** dim
    rng = np.random.default_rng(1)
    fields = {}
    for name in ("z", "p", "p2", "q", "x", "r"):
        f = m.field(g)
        m._chk(L.mgk_flat_fill(m.ctx, g.total, float(rng.uniform(0.1, 1.0)), f, None))
        fields[name] = f
    z, p, p2, q, x, r = (fields[k] for k in ("z", "p", "p2", "q", "x", "r"))
    ws, slot, t = C.c_void_p(), m.alloc(8), C.c_void_p()
    m._chk(L.mgk_cg_workspace_create(m.ctx, C.byref(ws)))
    m._chk(L.mgk_timer_create(m.ctx, C.byref(t)))
    coef, host = m.coef(COEF[dim]), C.c_double()
    beta, alpha = 0.37, 1e-3

    def direction_fused():
        m._chk(L.mgk_cg_direction_apply_dot_f64(m.ctx, C.byref(g), coef, beta, z, p, p2, q, ws, None, None))

    def direction_replaced():
        m._chk(L.mgk_flat_aypx(m.ctx, g.total, beta, z, p, None))
        m._chk(L.mgk_apply_f64(m.ctx, C.byref(g), coef, p, q, None))
        m._chk(L.mgk_flat_dot(m.ctx, g.total, p, q, C.byref(host), None))

    def update_fused():
        m._chk(L.mgk_cg_update_sumsq_f64(m.ctx, C.byref(g), alpha, p, q, x, r, ws, None, None))

    def update_replaced():
        m._chk(L.mgk_flat_axpy(m.ctx, g.total, alpha, p, x, None))
        m._chk(L.mgk_flat_axpy(m.ctx, g.total, -alpha, q, r, None))
        m._chk(L.mgk_sumsq_f64(m.ctx, C.byref(g), r, C.byref(host), None))

    def timed(fn, deferred):
        if deferred:
            m._chk(L.mgk_defer_result(m.ctx, slot))
        m._chk(L.mgk_timer_start(m.ctx, t, None))
        for _ in range(reps):
            fn()
        m._chk(L.mgk_timer_stop(m.ctx, t, None))
        ms = C.c_double()
        m._chk(L.mgk_timer_elapsed_ms(m.ctx, t, C.byref(ms)))
        if deferred:
            m._chk(L.mgk_defer_result(m.ctx, None))
        return ms.value

    row = {"dim": dim, "n": n, "unknowns": N, "samples": samples, "reps": reps}
    for name, fused, replaced, nbytes in (("direction", direction_fused, direction_replaced, 32), ("update", update_fused, update_replaced, 48)):
        timed(fused, False); timed(replaced, True)                           # warm-up
        a, b = [], []
        for _ in range(samples):
            a.append(timed(fused, False))
            b.append(timed(replaced, True))
        fa, fb = _stats(a, reps), _stats(b, reps)
        row[name] = {"fused": fa, "replaced": fb, "fused_over_replaced": fa["median_ms"] / fb["median_ms"],
                     "every_fused_sample_below_every_replaced_sample": fa["max_ms"] < fb["min_ms"],
                     "every_replaced_sample_below_every_fused_sample": fb["max_ms"] < fa["min_ms"],
                     "bytes_per_unknown": nbytes, "fused_GB/s": nbytes * N / (fa["median_ms"] * 1e-3) / 1e9}
    # the STREAM triad of bench.py (stream_ceiling), on three of the fields
    nn = int(g.total) & ~1
    best = 0.0
    for blocks in (256, 4096, 65536):
        for nt in (1, 0):
            m._chk(L.mgk_stream_triad_f64(m.ctx, nn, x, z, q, 0.5, blocks, nt, None))
            m._chk(L.mgk_timer_start(m.ctx, t, None))
            for _ in range(5):
                m._chk(L.mgk_stream_triad_f64(m.ctx, nn, x, z, q, 0.5, blocks, nt, None))
            m._chk(L.mgk_timer_stop(m.ctx, t, None))
            ms = C.c_double()
            m._chk(L.mgk_timer_elapsed_ms(m.ctx, t, C.byref(ms)))
            best = max(best, 24.0 * nn * 5 / (ms.value * 1e-3) / 1e9)
    row["stream_triad_GB/s"] = best
    for k in ("direction", "update"):
        row[k]["fused_over_triad"] = row[k]["fused_GB/s"] / best
    L.mgk_timer_destroy(m.ctx, t)
    L.mgk_cg_workspace_destroy(m.ctx, ws)
    for f in list(fields.values()) + [slot]:
        m.free(f)
    m.close()
    return row


def solves(dim, npts, scale, samples, kinds):
    from multigrid_petsc_amd.solver import Solver
    levels = (npts - 1).bit_length() - 1
    call = {"solve": lambda s: s.solve(), "gmres": lambda s: s.solve_gmres(30), "cg": lambda s: s.solve_cg()}
    S = {k: Solver(dim, npts, levels, v=(3, 3), scale=scale, maxiter=100, rtol=RTOL) for k in kinds}
    secs, its = {k: [] for k in kinds}, {}
    for k, s in S.items():
        s.set_rhs_problem()
        call[k](s)                                                        # warm-up: first launches, the graph recording, the allocations
    for _ in range(samples):
        for k, s in S.items():
            s.reset()
            its[k] = call[k](s)
            secs[k].append(s.solve_seconds)
    row = {"dim": dim, "npts": npts, "levels": levels, "scale": scale, "rtol": RTOL, "samples": samples}
    for k, s in S.items():
        rn = s.rnorm
        row[k] = {"iterations": its[k], "converged": bool(rn[-1] <= RTOL * s.bnorm), "relative_residual": float(rn[-1] / rn[0]),
                  "seconds": secs[k], "seconds_median": statistics.median(secs[k])}
        if k == "cg":
            row[k]["breakdown"] = s.cg_breakdown
        s.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["passes", "solves"])
    ap.add_argument("--shapes", default="2:4095,3:1023", help="passes: dim:n, comma separated")
    ap.add_argument("--cases", default="2:4097:0.8,2:4097:1.0,3:513:0.8,3:513:1.0", help="solves: dim:npts:scale, comma separated")
    ap.add_argument("--kinds", default="solve,gmres,cg")
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    specs = (a.shapes if a.mode == "passes" else a.cases).split(",")
    for spec in specs:
        f = spec.split(":")
        if a.mode == "passes":
            r = passes(int(f[0]), int(f[1]), a.samples or 7, a.reps)
        else:
            r = solves(int(f[0]), int(f[1]), float(f[2]), a.samples or 3, a.kinds.split(","))
        print(json.dumps(r), flush=True)
        rows.append(r)
        if a.out:
            with open(a.out, "w") as fo:
                for q in rows:
                    fo.write(json.dumps(q) + "\n")


if __name__ == "__main__":
    main()
