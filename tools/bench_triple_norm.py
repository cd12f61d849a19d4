#!/usr/bin/env python3
"""The gate of the 66-byte 3-D fine level (fuse bit 17; profiles/triple_norm/README.md): HIP-event timings of level 0's three passes at n^3 with
the coarse grid ((n - 1) / 2)^3, every pass timed alone and the three summed
    T_parent = mgk_prolong_jacobi2_f64 (k_pj2r3) + mgk_jacobi3_sumsq_mid_f64 (k_jacobi3s<4,2>) + mgk_sweep_residual_restrict_f64 (k_srr4b)    25 + 24 + 26 B
    T_new    = mgk_prolong_jacobi3_f64 (k_jacobi3s<4,0,PRO>) + mgk_jacobi3_sumsq_f64 (k_jacobi3s<4,1>) + mgk_residual_restrict_f64 (k_rrrow)  25 + 24 + 17 B
Random (separable) fields, not zero fields; best and median of 3 x 5 launches per pass.  T_parent is measured --repeat times (default 4); the
margin is the larger of 0.2 ms and three times the spread max - min of those sums, and it is fixed from the PARENT build's run (--save)
before T_new is looked at: the bit becomes part of the default at a width only if T_new <= T_parent - margin there.  The three-row form of
the norm pass (MGK_TUNE_J3S_NORM_R3 = 70) is timed beside the default one where the build has it.
usage: bench_triple_norm.py [n ...] [--root DIR] [--repeat K] [--save FILE] [--against FILE]
    --root DIR      the checkout whose multigrid_petsc_amd is measured
    --save FILE     write {n: [sums T_parent]} as JSON (run on the parent build)
    --against FILE  read such a file and print the verdict of the gate against it"""
import ctypes as C
import json
import os
import sys

import numpy as np

argv = sys.argv[1:]


def opt(name, default=None):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


root = os.path.abspath(opt("--root", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
repeat, save, against = int(opt("--repeat", "4")), opt("--save"), opt("--against")
sys.path.insert(0, root)
from multigrid_petsc_amd import mgk as mgk_module  # noqa: E402
from multigrid_petsc_amd.mgk import Mgk  # noqa: E402

R3 = getattr(mgk_module, "TUNE_J3S_NORM_R3", None)
sizes = [int(a) for a in argv] or [1023, 511]
m = Mgk(0)
L = m.L
t = C.c_void_p()
m._chk(L.mgk_timer_create(m.ctx, C.byref(t)))
ms, ss = C.c_double(), C.c_double()
saved = {}
parent = json.load(open(against)) if against else None


def timeit(fn, rounds=3, reps=5):
    fn()
    m.sync()
    per = []
    for _ in range(rounds):
        m._chk(L.mgk_timer_start(m.ctx, t, None))
        for _ in range(reps):
            fn()
        m._chk(L.mgk_timer_stop(m.ctx, t, None))
        m._chk(L.mgk_timer_elapsed_ms(m.ctx, t, C.byref(ms)))
        per.append(ms.value / reps)
    return min(per), sorted(per)[len(per) // 2]


for n in sizes:
    g, gc = m.geom(3, n), m.geom(3, (n - 1) // 2)
    G, GC = C.byref(g), C.byref(gc)
    rng = np.random.default_rng(n)
    r1 = [m.upload(rng.uniform(-1, 1, n)) for _ in range(3)]
    rc = [m.upload(rng.uniform(-1, 1, gc.nx)) for _ in range(3)]
    u, b, out, uc, bc = m.field(g), m.field(g), m.field(g), m.field(gc), m.field(gc)
    m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[0], r1[1], r1[2], u, None))
    m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[2], r1[0], r1[1], b, None))
    m._chk(L.mgk_fill_separable_f64(m.ctx, GC, rc[0], rc[1], rc[2], uc, None))
    q = float((n + 1) ** 2)
    coef, dinv, sc = m.coef([q, q, q, -6 * q, q, q, q]), -1.0 / (6 * q), 6.0 / 7.0
    dinvc = -1.0 / (6 * float(((n - 1) // 2 + 1) ** 2))
    N = float(n) ** 3
    passes = {
        "pj2  (P + S1, S2)        k_pj2r3": (25, lambda: L.mgk_prolong_jacobi2_f64(m.ctx, G, GC, coef, dinv, sc, b, uc, u, out, None)),
        "mid  (S3, N + S1', S2')  k_jacobi3s<4,2>": (24, lambda: L.mgk_jacobi3_sumsq_mid_f64(m.ctx, G, coef, dinv, sc, b, u, out, C.byref(ss), None)),
        "srr  (S3' + R)           k_srr4b": (26, lambda: L.mgk_sweep_residual_restrict_f64(m.ctx, G, GC, coef, dinv, sc, b, u, out, bc, None, dinvc, sc, None)),
        "pj3  (P + S1, S2, S3)    k_jacobi3s<4,0,PRO>": (25, lambda: L.mgk_prolong_jacobi3_f64(m.ctx, G, GC, coef, dinv, sc, b, uc, u, out, None)),
        "nrm  (N + S1', S2', S3') k_jacobi3s<4,1>": (24, lambda: L.mgk_jacobi3_sumsq_f64(m.ctx, G, coef, dinv, sc, b, u, out, C.byref(ss), None)),
        "rr   (R)                 k_rrrow": (17, lambda: L.mgk_residual_restrict_f64(m.ctx, G, GC, coef, b, u, bc, None)),
    }
    names = list(passes)
    OLD, NEW = names[:3], names[3:]

    def one(name, tag=""):
        nbytes, fn = passes[name]
        best, med = timeit(lambda: m._chk(fn()))
        print(f"n={n} {name}{tag}: best {best:7.3f} ms  median {med:7.3f} ms  {nbytes * N / best / 1e9:5.2f} TB/s of its {nbytes} B", flush=True)
        return best

    sums, tnew = [], None
    for k in range(repeat):
        s_old = sum(one(nm, f" run {k}") for nm in OLD)
        sums.append(s_old)
        print(f"n={n} T_parent run {k}: {s_old:.3f} ms", flush=True)
        if k == 0:      # the new passes between the repeats of the old ones: the same session, the same thermal state
            tnew = sum(one(nm) for nm in NEW)
            print(f"n={n} T_new: {tnew:.3f} ms", flush=True)
            if R3 is not None:
                L.mgk_set_tuning(int(R3), -1)
                try:
                    one(NEW[1], " three rows per wave (variant 70)")
                finally:
                    L.mgk_set_tuning(-1, -1)
    spread = max(sums) - min(sums)
    margin = max(0.2, 3 * spread)
    print(f"n={n} T_parent: min {min(sums):.3f} ms, max {max(sums):.3f} ms, spread {spread:.3f} ms, margin {margin:.3f} ms", flush=True)
    saved[str(n)] = sums
    print(f"n={n} this build: T_new {tnew:.3f} ms against its own T_parent {min(sums):.3f} ms - margin {margin:.3f} ms: "
          f"{'MET' if tnew <= min(sums) - margin else 'NOT met'}", flush=True)
    if parent and str(n) in parent:
        pb = parent[str(n)]
        pm = max(0.2, 3 * (max(pb) - min(pb)))
        print(f"n={n} GATE: T_new {tnew:.3f} ms against the parent build's T_parent {min(pb):.3f} ms - margin {pm:.3f} ms: "
              f"{'MET' if tnew <= min(pb) - pm else 'NOT met'}", flush=True)
    for p in r1 + rc + [u, b, out, uc, bc]:
        m.free(p)
if save:
    json.dump(saved, open(save, "w"))
L.mgk_timer_destroy(m.ctx, t)
m.close()
