#!/usr/bin/env python3
"""The 91-byte fine level on z-slabs (fuse bit 14; loopback ranks = threads) against the oracle: solve and the bench's fixed-count loop, overlap on / off.
MOCK=1 (default): over the host mock, small sizes; MOCK=0: on the GPU (cases like 513,5,4,255,255 = npts, levels, ranks, dist_min_n, pair_min_n; ';' separates cases).
usage: stress_slab91.py [cases] [problem|rhs]      ('' for cases = the default list)
Right-hand-side mode rhs: each run draws, from a generator of its own, a right-hand side of tests/rhs_cases.py (uniform / spikes, the spikes on both planes next to
every rank cut); each rank hands mg_solver_set_rhs_host its own planes [z0, z0 + nz) of the global b.  Half the runs then load a second right-hand side into the
live solvers (the neighbours' b ghost planes and far planes are caches of the first one) and compare with fresh solvers, bit for bit, and with the oracle."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
if os.environ.get("MOCK", "1") == "1":
    from stress_solver_mock import inject
    inject()
import numpy as np
from multigrid_petsc_amd.solver import Solver
from multigrid_petsc_amd.comm import LoopbackWorld
from oracle import Oracle
orc = Oracle()
FUSE = 63 | 256 | 512 | 1024 | 2048 | 4096 | 8192 | 16384
bad = 0
REFS = {}
cases = [(33, 4, 2, 7, 7), (33, 5, 2, 15, 7), (33, 4, 3, 7, 15), (65, 5, 2, 15, 15), (65, 6, 4, 7, 7), (65, 5, 3, 15, 31), (65, 4, 8, 7, 7)] if len(sys.argv) < 2 or not sys.argv[1] else [tuple(int(x) for x in c.split(",")) for c in sys.argv[1].split(";")]
RHS_MODE = sys.argv[2] if len(sys.argv) > 2 else "problem"
if RHS_MODE not in ("problem", "rhs"):
    sys.exit(f"right-hand-side mode {RHS_MODE!r}: problem or rhs")


def rhs_runs():
    """the rhs mode (see the module's docstring); returns the number of bad runs"""
    import rhs_cases
    rng2 = np.random.default_rng(0x736C6162)
    nbad = 0
    for npts, levels, P, dist, pair in cases:
        kw = dict(v=(3, 3), scale=6.0 / 7.0, maxiter=40, nranks=P, dist_min_n=dist, fuse=FUSE, pair_min_n=pair)

        def ranks(fn):
            world = LoopbackWorld(P)
            try:
                return world.run(fn)
            finally:
                world.close()

        def planes(rank, comm):
            s = Solver(3, npts, levels, rank=rank, comm=comm, **kw)
            r = s.level_planes(0)
            s.close()
            return r
        cuts = [z0 for z0, _ in ranks(planes)][1:]
        for overlap in (1, 0):
            for mode in ("solve", "cycles"):
                def oracle_run(b):
                    return orc.vcycle(3, npts, levels, 3, 3, maxiter=40, scale=6.0 / 7.0, fixed_cycles=0 if mode == "solve" else 5, b=b)

                def draw_b():
                    family = str(rng2.choice(rhs_cases.FAMILIES))
                    while True:
                        b = rhs_cases.make(family, 3, npts, int(rng2.integers(1 << 30)), cuts)
                        ref = oracle_run(b)
                        if mode == "cycles" or rhs_cases.stop_rule_clear(ref):          # (never skipped: another seed)
                            return family, b, ref
                (f1, b1, ref1), second = draw_b(), bool(rng2.integers(0, 2))
                f2, b2, ref2 = draw_b() if second else (None, None, None)

                def ops(s):
                    if mode == "solve":
                        it = s.solve()
                    else:
                        s.cycles(2); s.cycles(3); s.sync(); it = s.iterations
                    return it, s.solution(), s.rnorm, s.bnorm

                def mine(s, b):
                    z0, nz = s.level_planes(0)
                    n = npts - 2
                    return b.reshape(n, n * n)[z0:z0 + nz]

                def fn(rank, comm, bs):
                    s = Solver(3, npts, levels, rank=rank, comm=comm, overlap=overlap, **kw)
                    out = []
                    for b in bs:
                        s.set_rhs(mine(s, b))
                        out.append(ops(s))
                    s.close()
                    return out
                res = ranks(lambda rank, comm: fn(rank, comm, [b1, b2] if second else [b1]))
                fresh = ranks(lambda rank, comm: fn(rank, comm, [b2])) if second else None
                ok = True
                for q, ref in enumerate([ref1, ref2] if second else [ref1]):
                    u = np.concatenate([r[q][1] for r in res])
                    ok = ok and all(r[q][0] == ref["iters"] for r in res) and np.array_equal(u, ref["u"])
                    ok = ok and all(np.max(np.abs(r[q][2] - ref["rnorm"]) / ref["rnorm"]) < 1e-10 and abs(r[q][3] - ref["bnorm"]) <= 1e-12 * ref["bnorm"] for r in res)
                if second:
                    ok = ok and all(a[1][0] == f[0][0] and np.array_equal(a[1][1], f[0][1]) and np.array_equal(a[1][2], f[0][2]) and a[1][3] == f[0][3]
                                    for a, f in zip(res, fresh))
                print("OK " if ok else "BAD", npts, levels, P, dist, pair, "overlap", overlap, mode, "rhs", f1, ("then " + f2 + " on the live solvers") if second else "",
                      [r[-1][0] for r in res], (ref2 if second else ref1)["iters"], flush=True)
                nbad += 0 if ok else 1
    return nbad


if RHS_MODE == "rhs":
    bad = rhs_runs()
    print("bad", bad)
    sys.exit(1 if bad else 0)
for npts, levels, P, dist, pair in cases:
    for overlap in (1, 0):
        for mode in ("solve", "cycles"):
            world = LoopbackWorld(P)
            def fn(rank, comm):
                s = Solver(3, npts, levels, v=(3, 3), scale=6.0 / 7.0, maxiter=40, rank=rank, nranks=P, comm=comm, dist_min_n=dist, fuse=FUSE, pair_min_n=pair, overlap=overlap)
                s.set_rhs_problem()
                if mode == "solve":
                    it = s.solve()
                else:
                    s.cycles(2); s.cycles(3); s.sync(); it = s.iterations
                r = (it, s.solution(), s.rnorm)
                s.close()
                return r
            try:
                res = world.run(fn)
            finally:
                world.close()
            key = (npts, levels, mode)
            if key not in REFS:
                REFS[key] = orc.vcycle(3, npts, levels, 3, 3, maxiter=40, scale=6.0 / 7.0, fixed_cycles=0 if mode == "solve" else 5)
            ref = REFS[key]
            u = np.concatenate([r[1] for r in res])
            ok = all(r[0] == ref["iters"] for r in res) and np.array_equal(u, ref["u"]) and all(np.max(np.abs(r[2] - ref["rnorm"]) / ref["rnorm"]) < 1e-10 for r in res)
            print("OK " if ok else "BAD", npts, levels, P, dist, pair, "overlap", overlap, mode, [r[0] for r in res], ref["iters"], float(np.max(np.abs(u - ref["u"]))), flush=True)
            bad += 0 if ok else 1
print("bad", bad)
sys.exit(1 if bad else 0)
