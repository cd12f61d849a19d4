"""The three passes of CG over the fp32 cycle against the launches they replace, and whole solves: CG on a mixed solver against fp64 CG.  One GPU.

    python tools/bench_cg_mixed.py passes [--sizes 511,1023] [--samples 7] [--reps 5] [--out FILE]
    python tools/bench_cg_mixed.py solves [--cases 513:0.8,513:1.0,1025:0.8,1025:1.0] [--rhs manufactured|rough:SEED] [--samples 3] [--out FILE]

passes (3-D, n^3): HIP events round `reps` back-to-back launches, after a warm-up of each version; a fused pass and the launches it replaces
ALTERNATE within one process, sample by sample; no call synchronises with the host (the fused passes are given no host pointer, the replaced
reductions run under mgk_defer_result or without a host pointer).  Per size one JSON line: every sample, median, min and max of both
versions, the achieved bytes/s of the fused pass against its bytes per unknown, and whether EVERY fused sample lies below EVERY sample of
the replaced launches -- the bar a fused pass has to clear.  What is replaced is built from the kernels the library had before these passes:
  dot         mgk_cg_dot_f64_f32 (12 B)                  against  mgk_memset0 + mgk_correct_f64_from_f32 into the zeroed field + mgk_multi_dot_f64 (k = 1)
  direction   mgk_cg_direction_apply_dot_zf32_f64 (28 B)  against  the same conversion + mgk_cg_direction_apply_dot_f64
  update      mgk_cg_update_sumsq_f64_f32 with e0 (56 B)  against  mgk_cg_update_sumsq_f64 + mgk_residual_f64_to_f32_jz on a zero u
solves: per case (npts:scale, 3-D, all levels, V(3,3), rtol 1e-7; the manufactured right-hand side, or with --rhs rough:SEED values drawn
uniformly from (-1, 1), the kind of right-hand side the tests converge on) a mixed solver under solve_cg_mixed and an
fp64 solver under solve_cg in ONE process, the samples alternating after one warm-up of each; step counts, every sample of solve_seconds, and
the ratio of the medians."""
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
COEF = [-0.6, -1.3, -0.7, 11.3, -1.1, -0.9, -0.8]
DINV, SCALE = 1.0 / 11.3, 0.8


def _stats(ms, reps):
    per = [v / reps for v in ms]
    return {"ms": per, "median_ms": statistics.median(per), "min_ms": min(per), "max_ms": max(per)}


def passes(n, samples, reps):
    from multigrid_petsc_amd.mgk import Geom, Mgk, cg_mixed_sigs
    m = Mgk(0)
    L = m.L
    cg_mixed_sigs(L)
    g, g32 = m.geom(3, n), Geom()
    m._chk(L.mgk_geom_init_f32(C.byref(g32), 3, n, n, n))
    N = n ** 3
    rng = np.random.default_rng(1)
    f64 = {}
    for name in ("zc", "p", "p2", "q", "x", "r"):
        f = m.field(g)
        m._chk(L.mgk_flat_fill(m.ctx, g.total, float(rng.uniform(0.1, 1.0)), f, None))
        f64[name] = f
    zc, p, p2, q, x, r = (f64[k] for k in ("zc", "p", "p2", "q", "x", "r"))
    zero = m.field(g)                                                      # the zero u of the replaced update's bridge pass
    z32, r32, e0 = (m.alloc(4 * g32.total) for _ in range(3))
    m._chk(L.mgk_residual_f64_to_f32_jz(m.ctx, C.byref(g), C.byref(g32), m.coef(COEF), p, zero, z32, e0, DINV, SCALE, C.byref(C.c_double()), None))   # z32 = (float) p
    ws, slot, t = C.c_void_p(), m.alloc(8), C.c_void_p()
    m._chk(L.mgk_cg_workspace_create(m.ctx, C.byref(ws)))
    m._chk(L.mgk_timer_create(m.ctx, C.byref(t)))
    coef, host = m.coef(COEF), C.c_double()
    rv = (C.c_void_p * 1)(r)
    beta, alpha = 0.37, 1e-3
    nbytes64 = 8 * g.total

    def convert():
        m._chk(L.mgk_memset0(m.ctx, zc, nbytes64, None))
        m._chk(L.mgk_correct_f64_from_f32(m.ctx, C.byref(g), C.byref(g32), z32, zc, None))

    def dot_fused():
        m._chk(L.mgk_cg_dot_f64_f32(m.ctx, C.byref(g), C.byref(g32), r, z32, ws, None, None))

    def dot_replaced():
        convert()
        m._chk(L.mgk_multi_dot_f64(m.ctx, C.byref(g), 1, rv, zc, slot, None, None))

    def direction_fused():
        m._chk(L.mgk_cg_direction_apply_dot_zf32_f64(m.ctx, C.byref(g), C.byref(g32), coef, beta, z32, p, p2, q, ws, None, None))

    def direction_replaced():
        convert()
        m._chk(L.mgk_cg_direction_apply_dot_f64(m.ctx, C.byref(g), coef, beta, zc, p, p2, q, ws, None, None))

    def update_fused():
        m._chk(L.mgk_cg_update_sumsq_f64_f32(m.ctx, C.byref(g), C.byref(g32), alpha, p, q, x, r, r32, e0, DINV, SCALE, ws, None, None))

    def update_replaced():
        m._chk(L.mgk_cg_update_sumsq_f64(m.ctx, C.byref(g), alpha, p, q, x, r, ws, None, None))
        m._chk(L.mgk_residual_f64_to_f32_jz(m.ctx, C.byref(g), C.byref(g32), coef, r, zero, r32, e0, DINV, SCALE, C.byref(host), None))

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

    row = {"dim": 3, "n": n, "unknowns": N, "samples": samples, "reps": reps}
    for name, fused, replaced, nbytes in (("dot", dot_fused, dot_replaced, 12), ("direction", direction_fused, direction_replaced, 28),
                                          ("update", update_fused, update_replaced, 56)):
        timed(fused, False); timed(replaced, True)                           # warm-up
        a, b = [], []
        for _ in range(samples):
            a.append(timed(fused, False))
            b.append(timed(replaced, True))
        fa, fb = _stats(a, reps), _stats(b, reps)
        row[name] = {"fused": fa, "replaced": fb, "fused_over_replaced": fa["median_ms"] / fb["median_ms"],
                     "every_fused_sample_below_every_replaced_sample": fa["max_ms"] < fb["min_ms"],
                     "bytes_per_unknown": nbytes, "fused_GB/s": nbytes * N / (fa["median_ms"] * 1e-3) / 1e9}
    L.mgk_timer_destroy(m.ctx, t)
    L.mgk_cg_workspace_destroy(m.ctx, ws)
    for f in list(f64.values()) + [zero, z32, r32, e0, slot]:
        m.free(f)
    m.close()
    return row


def solves(npts, scale, samples, rhs):
    from multigrid_petsc_amd.solver import Solver
    levels = (npts - 1).bit_length() - 1
    call = {"cg_mixed": lambda s: s.solve_cg_mixed(), "cg_fp64": lambda s: s.solve_cg()}
    S = {"cg_mixed": Solver(3, npts, levels, v=(3, 3), scale=scale, maxiter=100, rtol=RTOL, precision="mixed"),
         "cg_fp64": Solver(3, npts, levels, v=(3, 3), scale=scale, maxiter=100, rtol=RTOL)}
    secs, its = {k: [] for k in S}, {}
    b = None
    if rhs != "manufactured":
        b = np.random.default_rng(int(rhs.split(":")[1])).uniform(-1.0, 1.0, (npts - 2) ** 3)
    for k, s in S.items():
        if b is None:
            s.set_rhs_problem()
        else:
            s.set_rhs(b)
        call[k](s)                                                        # warm-up: first launches, the graph recording, the allocations
    for _ in range(samples):
        for k, s in S.items():
            s.reset()
            its[k] = call[k](s)
            secs[k].append(s.solve_seconds)
    row = {"dim": 3, "npts": npts, "levels": levels, "scale": scale, "rhs": rhs, "rtol": RTOL, "samples": samples}
    for k, s in S.items():
        rn = s.rnorm
        row[k] = {"iterations": its[k], "converged": bool(rn[-1] <= RTOL * s.bnorm), "relative_residual": float(rn[-1] / rn[0]),
                  "seconds": secs[k], "seconds_median": statistics.median(secs[k]), "breakdown": s.cg_breakdown}
        s.close()
    row["mixed_over_fp64"] = row["cg_mixed"]["seconds_median"] / row["cg_fp64"]["seconds_median"]
    row["every_mixed_sample_below_every_fp64_sample"] = max(row["cg_mixed"]["seconds"]) < min(row["cg_fp64"]["seconds"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["passes", "solves"])
    ap.add_argument("--sizes", default="511,1023", help="passes: n of the n^3 box, comma separated")
    ap.add_argument("--cases", default="513:0.8,513:1.0,1025:0.8,1025:1.0", help="solves: npts:scale, comma separated")
    ap.add_argument("--rhs", default="manufactured", help="solves: manufactured or rough:SEED")
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for spec in (a.sizes if a.mode == "passes" else a.cases).split(","):
        if a.mode == "passes":
            r = passes(int(spec), a.samples or 7, a.reps)
        else:
            f = spec.split(":")
            r = solves(int(f[0]), float(f[1]), a.samples or 3, a.rhs)
        print(json.dumps(r), flush=True)
        rows.append(r)
        if a.out:
            with open(a.out, "w") as fo:
                for q in rows:
                    fo.write(json.dumps(q) + "\n")


if __name__ == "__main__":
    main()
