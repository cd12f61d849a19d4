#!/usr/bin/env python3
"""The gate of the stacked 3-D pass's tile order and load policies (profiles/stacked_l2/README.md): HIP-event timings of the two level-0
passes that k_jacobi3s makes in a cycle with fuse bit 17, each timed alone at n^3 with the coarse grid ((n - 1) / 2)^3, and their sum
    T = mgk_prolong_jacobi3_f64 (k_jacobi3s<4,0,PRO>) + mgk_jacobi3_sumsq_f64 (k_jacobi3s<4,1>)
Random (separable) fields, best and median of 3 x 5 launches per pass, as tools/bench_triple_norm.py.  T is measured --repeat times (default
4) under the build's default tuning; the margin is the larger of 0.2 ms and three times the spread max - min of those sums.  It is fixed from
the PARENT build's run (--save) before this build's numbers are looked at: a variant becomes the default at a width only if its
T <= min T_parent - margin there, and at the other width it must not lie more than that width's margin above the parent's slowest repeat.
usage: bench_j3s_order.py [n ...] [--root DIR] [--repeat K] [--variants V,V,...] [--save FILE] [--against FILE]
    --root DIR        the checkout whose multigrid_petsc_amd is measured
    --variants LIST   first arguments of mgk_set_tuning to time T under, once each, between the repeats of the default
    --save FILE       write {n: [sums T]} as JSON (run on the parent build)
    --against FILE    read such a file and print the verdict of the gate against it"""
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
variants = [int(v) for v in opt("--variants", "").split(",") if v]
sys.path.insert(0, root)
from multigrid_petsc_amd.mgk import Mgk  # noqa: E402

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
    u, b, out, uc = m.field(g), m.field(g), m.field(g), m.field(gc)
    m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[0], r1[1], r1[2], u, None))
    m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[2], r1[0], r1[1], b, None))
    m._chk(L.mgk_fill_separable_f64(m.ctx, GC, rc[0], rc[1], rc[2], uc, None))
    q = float((n + 1) ** 2)
    coef, dinv, sc = m.coef([q, q, q, -6 * q, q, q, q]), -1.0 / (6 * q), 6.0 / 7.0
    N = float(n) ** 3
    passes = {
        "pj3  (P + S1, S2, S3)    k_jacobi3s<4,0,PRO>": (25, lambda: L.mgk_prolong_jacobi3_f64(m.ctx, G, GC, coef, dinv, sc, b, uc, u, out, None)),
        "nrm  (N + S1', S2', S3') k_jacobi3s<4,1>": (24, lambda: L.mgk_jacobi3_sumsq_f64(m.ctx, G, coef, dinv, sc, b, u, out, C.byref(ss), None)),
    }

    def one(name, tag=""):
        nbytes, fn = passes[name]
        best, med = timeit(lambda: m._chk(fn()))
        print(f"n={n} {name}{tag}: best {best:7.3f} ms  median {med:7.3f} ms  {nbytes * N / best / 1e9:5.2f} TB/s of its {nbytes} B", flush=True)
        return best

    def total(tag):
        s = sum(one(nm, tag) for nm in passes)
        print(f"n={n} T{tag}: {s:.3f} ms", flush=True)
        return s

    sums, tvar = [], {}
    for k in range(repeat):
        sums.append(total(f" default run {k}"))
        # the variants between the repeats of the default: the same session, the same thermal state
        for v in variants[k::repeat]:
            L.mgk_set_tuning(v, -1)
            try:
                tvar[v] = total(f" variant {v}")
            finally:
                L.mgk_set_tuning(-1, -1)
    spread = max(sums) - min(sums)
    margin = max(0.2, 3 * spread)
    print(f"n={n} T default: min {min(sums):.3f} ms, max {max(sums):.3f} ms, spread {spread:.3f} ms, margin {margin:.3f} ms", flush=True)
    saved[str(n)] = sums
    if parent and str(n) in parent:
        pb = parent[str(n)]
        pm = max(0.2, 3 * (max(pb) - min(pb)))
        for tag, tv in [("default", min(sums))] + [(f"variant {v}", tvar[v]) for v in variants]:
            print(f"n={n} GATE {tag}: T {tv:.3f} ms against the parent build's {min(pb):.3f} .. {max(pb):.3f} ms, margin {pm:.3f} ms: "
                  f"faster by the margin: {'MET' if tv <= min(pb) - pm else 'NOT met'}; "
                  f"slower than the parent: {'YES' if tv > max(pb) + pm else 'no'}", flush=True)
    for p in r1 + rc + [u, b, out, uc]:
        m.free(p)
if save:
    json.dump(saved, open(save, "w"))
L.mgk_timer_destroy(m.ctx, t)
m.close()
