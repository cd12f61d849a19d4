#!/usr/bin/env python3
"""The gate of the prolongation + three-sweep pass (profiles/triple_prolong/README.md): HIP-event timings at n^3 with the coarse grid
((n - 1) / 2)^3 of
    T_old = mgk_prolong_jacobi_f64 + mgk_jacobi2_f64     (P + S1)(S2, S3): the two passes of the generic post-smoothing, timed as one sequence
    T_new = mgk_prolong_jacobi3_f64                      (P + S1, S2, S3): the one pass
Random (separable) fields, not zero fields; best and median of 3 x 5 launches; T_old is measured --repeat times (default 4) and the spread
max - min of its bests is printed: the pass is wired at a size only if T_new is below the PARENT build's T_old by more than that spread.
usage: bench_triple_prolong.py [n ...] [--root DIR] [--repeat K] [--save FILE] [--against FILE]
    --root DIR      the checkout whose multigrid_petsc_amd is measured (a build without the new entry point reports T_old alone)
    --save FILE     write {n: [bests of T_old]} as JSON (run on the parent build)
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
from multigrid_petsc_amd.mgk import Mgk  # noqa: E402

sizes = [int(a) for a in argv] or [511, 1023]
m = Mgk(0)
L = m.L
t = C.c_void_p()
m._chk(L.mgk_timer_create(m.ctx, C.byref(t)))
ms = C.c_double()
have_new = hasattr(L, "mgk_prolong_jacobi3_f64")
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
    u, b, tmp, out, uc = m.field(g), m.field(g), m.field(g), m.field(g), m.field(gc)
    m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[0], r1[1], r1[2], u, None))
    m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[2], r1[0], r1[1], b, None))
    m._chk(L.mgk_fill_separable_f64(m.ctx, GC, rc[0], rc[1], rc[2], uc, None))
    q = float((n + 1) ** 2)
    coef, dinv, sc = m.coef([q, q, q, -6 * q, q, q, q]), -1.0 / (6 * q), 6.0 / 7.0
    N = float(n) ** 3

    def old():
        m._chk(L.mgk_prolong_jacobi_f64(m.ctx, G, GC, coef, dinv, sc, b, uc, u, tmp, None))
        m._chk(L.mgk_jacobi2_f64(m.ctx, G, coef, dinv, sc, b, tmp, out, None))

    def new():
        m._chk(L.mgk_prolong_jacobi3_f64(m.ctx, G, GC, coef, dinv, sc, b, uc, u, out, None))

    bests = []
    for k in range(repeat):
        best, med = timeit(old)
        bests.append(best)
        print(f"n={n} T_old (P + S1)(S2, S3), run {k}: best {best:7.3f} ms  median {med:7.3f} ms  {49 * N / best / 1e9:5.2f} TB/s of its 49 B", flush=True)
        if have_new and k == 0:      # the new pass between the repeats of the old ones: the same session, the same thermal state
            for var, zc in ((-1, -1), (68, -1), (65, -1)):
                L.mgk_set_tuning(var, zc)
                try:
                    nb, nm = timeit(new)
                finally:
                    L.mgk_set_tuning(-1, -1)
                print(f"n={n} T_new (P + S1, S2, S3) variant {var:3d}: best {nb:7.3f} ms  median {nm:7.3f} ms  {25 * N / nb / 1e9:5.2f} TB/s of its 25 B", flush=True)
                if var == -1:
                    tnew = nb
    spread = max(bests) - min(bests)
    print(f"n={n} T_old: min {min(bests):.3f} ms, max {max(bests):.3f} ms, spread {spread:.3f} ms", flush=True)
    saved[str(n)] = bests
    if have_new:
        print(f"n={n} this build: T_new {tnew:.3f} ms against T_old {min(bests):.3f} ms - spread {spread:.3f} ms: "
              f"{'MET' if tnew < min(bests) - spread else 'NOT met'}", flush=True)
        if parent and str(n) in parent:
            pb = parent[str(n)]
            ps = max(pb) - min(pb)
            print(f"n={n} GATE: T_new {tnew:.3f} ms against the parent build's T_old {min(pb):.3f} ms - spread {ps:.3f} ms: "
                  f"{'MET' if tnew < min(pb) - ps else 'NOT met'}", flush=True)
    for p in r1 + rc + [u, b, tmp, out, uc]:
        m.free(p)
if save:
    json.dump(saved, open(save, "w"))
L.mgk_timer_destroy(m.ctx, t)
m.close()
