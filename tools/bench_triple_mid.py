#!/usr/bin/env python3
"""The gate of the 75-byte fine level's middle pass (profiles/triple_mid/README.md): HIP-event timings at n^3 (default 1023) of the stacked
three-sweep pass (mgk_jacobi3_sumsq_mid_f64 and the stacked form of mgk_jacobi3_f64 / _sumsq_f64) beside the passes it would replace --
the two-sweep pass plain and with the mid norm, residual + restriction, sweep + residual + restriction.  Random (separable) fields, not zero
fields; best and median of 3 x 5 launches.  Prints the break-even T* = t(mid-norm pair) + t(pair) + t(residual+restriction) - t(sweep+residual+
restriction) of the build it runs on.
usage: bench_triple_mid.py [n] [--root DIR]     (--root: the checkout whose multigrid_petsc_amd is measured; a build that lacks the new entry
points reports the old passes alone)"""
import ctypes as C
import os
import sys

import numpy as np

argv = sys.argv[1:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in argv:
    i = argv.index("--root")
    root = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
sys.path.insert(0, root)
from multigrid_petsc_amd.mgk import Mgk  # noqa: E402

n = int(argv[0]) if argv else 1023
m = Mgk(0)
L = m.L
g, gc = m.geom(3, n), m.geom(3, (n - 1) // 2)
G, GC = C.byref(g), C.byref(gc)
rng = np.random.default_rng(0)
r1 = [m.upload(rng.uniform(-1, 1, n)) for _ in range(3)]
u, b, out, bc, uc = m.field(g), m.field(g), m.field(g), m.field(gc), m.field(gc)
m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[0], r1[1], r1[2], u, None))
m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[2], r1[0], r1[1], b, None))
q = float((n + 1) ** 2)
coef, dinv, sc = m.coef([q, q, q, -6 * q, q, q, q]), -1.0 / (6 * q), 6.0 / 7.0
ss = C.c_double()
t = C.c_void_p()
m._chk(L.mgk_timer_create(m.ctx, C.byref(t)))
ms = C.c_double()
N = float(n) ** 3


def timeit(fn, rounds=3, reps=5):
    m._chk(fn())
    m.sync()
    per = []
    for _ in range(rounds):
        m._chk(L.mgk_timer_start(m.ctx, t, None))
        for _ in range(reps):
            m._chk(fn())
        m._chk(L.mgk_timer_stop(m.ctx, t, None))
        m._chk(L.mgk_timer_elapsed_ms(m.ctx, t, C.byref(ms)))
        per.append(ms.value / reps)
    return min(per), sorted(per)[len(per) // 2]


def report(name, fn, nbytes, var=-1, zc=-1):
    L.mgk_set_tuning(var, zc)
    try:
        best, med = timeit(fn)
    finally:
        L.mgk_set_tuning(-1, -1)
    print(f"n={n} {name:44s} variant {var:3d} zc {zc:4d}: best {best:7.3f} ms  median {med:7.3f} ms  {nbytes * N / best / 1e9:5.2f} TB/s of its {nbytes} B", flush=True)
    return best


pair = report("two sweeps (k_jacobi2r)", lambda: L.mgk_jacobi2_f64(m.ctx, G, coef, dinv, sc, b, u, out, None), 24)
pairm = report("two sweeps + mid norm (k_jacobi2r<..,2>)", lambda: L.mgk_jacobi2_sumsq_mid_f64(m.ctx, G, coef, dinv, sc, b, u, out, C.byref(ss), None), 24)
rr = report("residual + restriction + coarse sweep (k_rrrow)", lambda: L.mgk_residual_restrict_jz_f64(m.ctx, G, GC, coef, b, u, bc, uc, dinv, sc, None), 18)
srr = report("sweep + residual + restriction (k_srr4b)",
             lambda: L.mgk_sweep_residual_restrict_f64(m.ctx, G, GC, coef, dinv, sc, b, u, out, bc, uc, dinv, sc, None), 26)
tstar = pairm + pair + rr - srr
print(f"n={n} break-even T* = {pairm:.3f} + {pair:.3f} + {rr:.3f} - {srr:.3f} = {tstar:.3f} ms; gate T* - 0.6 = {tstar - 0.6:.3f} ms", flush=True)
report("three sweeps, independent waves (k_jacobi3_3d)", lambda: L.mgk_jacobi3_f64(m.ctx, G, coef, dinv, sc, b, u, out, None), 24, 66 if hasattr(L, "mgk_jacobi3_sumsq_mid_f64") else -1)
if hasattr(L, "mgk_jacobi3_sumsq_mid_f64"):
    mid = lambda: L.mgk_jacobi3_sumsq_mid_f64(m.ctx, G, coef, dinv, sc, b, u, out, C.byref(ss), None)
    best = min(report("three sweeps + mid norm, stacked (k_jacobi3s)", mid, 24, var, zc)
               for var, zc in ((-1, -1), (68, -1), (65, -1), (-1, 64), (-1, 128), (-1, 256), (-1, 512)))
    report("three sweeps, stacked (k_jacobi3s)", lambda: L.mgk_jacobi3_f64(m.ctx, G, coef, dinv, sc, b, u, out, None), 24, 67)
    report("three sweeps + input norm, stacked, 3 rows", lambda: L.mgk_jacobi3_sumsq_f64(m.ctx, G, coef, dinv, sc, b, u, out, C.byref(ss), None), 24, 67)
    print(f"n={n} mid form, best setting: {best:.3f} ms against the gate {tstar - 0.6:.3f} ms: {'MET' if best <= tstar - 0.6 else 'NOT met'}", flush=True)
L.mgk_timer_destroy(m.ctx, t)
m.close()
