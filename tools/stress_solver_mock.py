#!/usr/bin/env python3
"""tools/stress_solver.py on the CPU: the PRODUCT's host logic (csrc/mg_solver.c, unchanged) over tests/mock_mgk.cpp (the kernel ABI in host
memory, canonical arithmetic) with configurations drawn at random against the oracle -- sweep counts, depth, damping, fuse bits, pair
threshold, recording on / off, precision.  What it can find is what the host decides: which pass runs when, buffer swaps, the coarse-level
recording, deferred sweeps (the odd-swap hole of the recording, round 3, shows here exactly as on the GPU).  Small sizes only: the mock is
scalar host code.  Test infrastructure: the mock library is injected into the package's loader cache HERE; the product has no such switch.
usage: stress_solver_mock.py [count] [seed] [problem|rhs]
The third argument is the right-hand-side mode.  problem (default): the manufactured right-hand side (mg_solver_set_rhs_problem), every draw as it has
always been.  rhs: the same draws, and from a SEPARATE generator a right-hand side of tests/rhs_cases.py (rough uniform data / a handful of spikes)
loaded through mg_solver_set_rhs_host; half the draws then load a second, different right-hand side into the same, live solver object -- or go from the
manufactured one to a host one or back -- and compare the second result with a fresh solver's (bit for bit, norms included) and with the oracle's.
usage: stress_solver_mock.py count seed problem|rhs offwidth
The optional fourth argument swaps the size lists: every draw above takes npts = 2^k + 1; with `offwidth` npts - 1 is 3, 5 or 7 times a power of two
(level widths 11, 23, 47, 95, ...: rows that are no whole number of wave rows, or a number of them that no block width matches) and the depth is
drawn up to the deepest hierarchy mg_solver_create accepts for that size.  Without it every draw is what it has always been."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_mock():
    out = os.path.join(ROOT, "tests", "_san")
    os.makedirs(out, exist_ok=True)
    inc = "-I" + os.path.join(ROOT, "include")
    objs = []
    for cc, std, src, obj in (("g++", "-std=c++17", os.path.join(ROOT, "tests", "mock_mgk.cpp"), "stress_mock_mgk.o"),
                              ("gcc", "-std=c99", os.path.join(ROOT, "multigrid_petsc_amd", "csrc", "mg_solver.c"), "stress_mg_solver.o"),
                              ("gcc", "-std=c99", os.path.join(ROOT, "multigrid_petsc_amd", "csrc", "mg_comm.c"), "stress_mg_comm.o")):
        o = os.path.join(out, obj)
        subprocess.run([cc, std, "-O2", "-fPIC", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L", inc, "-c", src, "-o", o], check=True)
        objs.append(o)
    so = os.path.join(out, "libmgsolve_stress.so")
    subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread", "-ldl"], check=True)
    return so


def inject():
    """build the mock-backed library and make the package's loader hand it out (before multigrid_petsc_amd.solver / .comm are imported)"""
    import multigrid_petsc_amd._lib as loader
    lib = ctypes.CDLL(build_mock(), mode=ctypes.RTLD_GLOBAL)
    loader._cache["mgk"] = lib
    loader._cache["mgpetsc"] = lib


def rhs_draw(rng2, rhs_cases, Solver, kw, mode, k1, k2, oracle_run, same, tag):
    """one draw of the rhs mode; returns 1 on a mismatch.  The right-hand sides come from rng2 alone (the configuration's generator is not touched).
    A draw that runs to the tolerance takes a right-hand side on which the ORACLE's stop decision is not near a tie: another seed is drawn until it is."""
    dim, npts = kw["dim"], kw["npts"]

    def draw_b():
        kind = str(rng2.choice(["uniform", "spikes", "problem"], p=[0.4, 0.4, 0.2]))
        if kind == "spikes" and npts < rhs_cases.spikes_min_npts(dim):
            kind = "uniform"
        while True:
            b = None if kind == "problem" else rhs_cases.make(kind, dim, npts, int(rng2.integers(1 << 30)))
            if mode == "cycles" or rhs_cases.stop_rule_clear(oracle_run(0, b)):
                return kind, b
            if kind == "problem":                      # (nothing to redraw: the manufactured mode itself sits on the threshold here)
                kind = "uniform"

    def load(s, b):
        if b is None:
            s.set_rhs_problem()
        else:
            s.set_rhs(b)

    def ops(s):
        """what the problem mode does with a solver, on whatever right-hand side it holds: [(fixed count or 0, iterations, u, history, ||b||)]"""
        out = []
        if mode != "solve":
            s.cycles(k1)
            if k2:
                s.cycles(k2)
            s.sync()
            out.append((k1 + k2, s.iterations, s.solution(), s.rnorm, s.bnorm))
            if mode == "cycles+solve":
                s.reset()
        if mode != "cycles":
            it = s.solve()
            out.append((0, it, s.solution(), s.rnorm, s.bnorm))
        return out

    (kind1, b1), second = draw_b(), bool(rng2.integers(0, 2))
    kind2, b2 = draw_b() if second else (None, None)
    if second and kind1 == "problem" and kind2 == "problem":
        kind2, b2 = "uniform", None
        while b2 is None or not (mode == "cycles" or rhs_cases.stop_rule_clear(oracle_run(0, b2))):
            b2 = rhs_cases.make("uniform", dim, npts, int(rng2.integers(1 << 30)))
    tag = f"{tag} rhs {kind1}" + (f" then {kind2} on the live solver" if second else "")
    try:
        s = Solver(**kw)
        load(s, b1)
        first = ops(s)
        live = fresh = None
        if second:
            load(s, b2)
            live = ops(s)
        s.close()
        if second:
            s = Solver(**kw)
            load(s, b2)
            fresh = ops(s)
            s.close()
    except Exception as e:
        print("REFUSED", tag, str(e)[:120], flush=True)
        return 0
    for b, results in ((b1, first), (b2, live)):
        for fixed, it, u, rn, bn in results or []:
            ref = oracle_run(fixed, b)
            if not (same(it, u, rn, ref) and abs(bn - ref["bnorm"]) <= 1e-12 * ref["bnorm"]):
                print("MISMATCH", tag, f"(leg: {'fixed ' + str(fixed) if fixed else 'solve'}, {'second' if results is live else 'first'} right-hand side)",
                      "iters", it, ref["iters"], "max|du|", float(np.max(np.abs(u - ref["u"]))), flush=True)
                return 1
    if second:
        for (fa, ia, ua, ra, ba), (fb, ib, ub, rb, bb) in zip(live, fresh):
            if not (ia == ib and ba == bb and np.array_equal(ua, ub) and np.array_equal(ra, rb)):
                print("MISMATCH", tag, "(the live solver against a fresh one)", "iters", ia, ib, "max|du|", float(np.max(np.abs(ua - ub))), flush=True)
                return 1
    return 0


def main(mock=True):
    """mock=False: the same draws on the GPU over the real libraries, with the larger sizes (tools/stress_solver.py)"""
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    rhs_mode = sys.argv[3] if len(sys.argv) > 3 else "problem"
    if rhs_mode not in ("problem", "rhs"):
        sys.exit(f"right-hand-side mode {rhs_mode!r}: problem or rhs")
    rng2 = np.random.default_rng([int(sys.argv[2]) if len(sys.argv) > 2 else 1, 0x726873]) if rhs_mode == "rhs" else None
    offwidth = len(sys.argv) > 4
    if offwidth and sys.argv[4] != "offwidth":
        sys.exit(f"size lists {sys.argv[4]!r}: offwidth, or nothing")
    if mock:
        inject()
    rhs_cases = __import__("rhs_cases") if rhs_mode == "rhs" else None      # (tests/rhs_cases.py: the rhs mode alone needs it)
    from multigrid_petsc_amd.solver import Solver
    from oracle import Oracle
    orc = Oracle()
    bad = 0
    for q in range(count):
        dim = int(rng.choice([2, 3, 3]))
        if offwidth:
            if mock:
                npts = int(rng.choice([13, 25, 41, 49, 57, 81, 97] if dim == 2 else [13, 21, 25]))
            else:
                npts = int(rng.choice([13, 25, 41, 49, 97, 193, 385, 641, 769, 897] if dim == 2 else [13, 21, 25, 49, 97]))
            lmax = 0                                         # the deepest hierarchy mg_solver_create takes: every level an odd width >= 1
            while (npts - 1) % (1 << lmax) == 0 and ((npts - 1) >> lmax) - 1 >= 1 and (((npts - 1) >> lmax) - 1) & 1:
                lmax += 1
        elif mock:
            npts = int(rng.choice([9, 17, 33, 65, 129] if dim == 2 else [9, 17, 33]))
            lmax = int(np.log2(npts - 1))
        else:
            npts = int(rng.choice([9, 17, 33, 65, 129, 257, 513, 1025] if dim == 2 else [9, 17, 33, 65, 129]))
            lmax = int(np.log2(npts - 1))
        levels = int(rng.integers(1, lmax + 1))
        v0, v1 = int(rng.integers(0, 6)), int(rng.integers(1, 5))
        mesh = int(rng.choice([0, 0, 1, 2])) if dim == 2 else 0
        scale = float(rng.choice([0.8, 1.0, 6.0 / 7.0, 0.5]))
        fuse = int(rng.choice([-1, -1, 0, 32, 63, 63 | 256 | 512, 63 | 256 | 512 | 1024 | 2048, 63 | 256 | 512 | 8192, int(rng.integers(0, 16384)),
                               int(rng.integers(0, 16384)) | 32]))
        pair = int(rng.choice([0, 7, 7, 15, 31]))
        graph = int(rng.choice([-1, -1, 0]))
        prec = str(rng.choice(["fp64", "fp64", "mixed"])) if dim == 3 else "fp64"
        if v0 == 0 and levels > 1:
            v0 = 1
        # what is done with the solver: solve to the tolerance | the bench's loop (fixed count, norms deferred, in one or two calls) followed
        # by a reset and a solve on the same handle | the same with the counts the other way round
        mode = str(rng.choice(["solve", "solve", "cycles", "cycles+solve"]))
        k1, k2 = int(rng.integers(1, 5)), int(rng.integers(0, 4))
        cheb = dim == 2 and mesh == 0 and prec == "fp64" and bool(rng.integers(0, 4) == 0)
        if v1 == 0 and cheb:
            v1 = 1
        kso = dict(ksp_type="chebyshev", eigenvalues=(0.2, 2.0)) if cheb else {}
        kor = dict(ksp_type=1, emin=0.2, emax=2.0) if cheb else {}
        tag = (f"dim={dim} npts={npts} levels={levels} v=({v0},{v1}) mesh={mesh} scale={scale:.4f} fuse={fuse} pair_min_n={pair} graph={graph} {prec} "
               f"{'chebyshev ' if cheb else ''}{mode} {k1}+{k2}")

        def oracle_run(fixed, b=None):
            kb = {} if b is None else dict(b=b)            # (the manufactured right-hand side: the call as it has always been)
            if prec == "mixed":
                return orc.vcycle_mixed(npts, levels, v0, v1, maxiter=max(40, fixed), scale=scale, fixed_cycles=fixed, **kb)
            return orc.vcycle(dim, npts, levels, v0, v1, maxiter=max(40, fixed), scale=scale, use_csr=1 if mesh else 0, mesh=mesh, fixed_cycles=fixed, **kb, **kor)

        def same(it, u, rn, ref):
            return (it == ref["iters"] and np.array_equal(u, ref["u"]) and
                    np.max(np.abs(rn - ref["rnorm"]) / np.maximum(ref["rnorm"], 1e-300)) <= 1e-10)
        if rhs_mode == "rhs":
            bad += rhs_draw(rng2, rhs_cases, Solver, dict(dim=dim, npts=npts, levels=levels, v=(v0, v1), maxiter=40, scale=scale, fuse=fuse, pair_min_n=pair,
                                                          mesh=mesh, graph=graph, precision=prec, **kso), mode, k1, k2, oracle_run, same, tag)
            continue
        try:
            s = Solver(dim, npts, levels, v=(v0, v1), maxiter=40, scale=scale, fuse=fuse, pair_min_n=pair, mesh=mesh, graph=graph, precision=prec, **kso)
            s.set_rhs_problem()
            results = []
            if mode != "solve":
                s.cycles(k1)
                if k2:
                    s.cycles(k2)
                s.sync()
                results.append((k1 + k2, s.iterations, s.solution(), s.rnorm))
                if mode == "cycles+solve":
                    s.reset()
            if mode != "cycles":
                it = s.solve()
                results.append((0, it, s.solution(), s.rnorm))
            s.close()
        except Exception as e:                               # a configuration the solver refuses is reported, not counted as a mismatch
            print("REFUSED", tag, str(e)[:120], flush=True)
            continue
        for fixed, it, u, rn in results:
            ref = oracle_run(fixed)
            if not same(it, u, rn, ref):
                bad += 1
                print("MISMATCH", tag, f"(leg: {'fixed ' + str(fixed) if fixed else 'solve'})", "iters", it, ref["iters"], "max|du|", float(np.max(np.abs(u - ref["u"]))),
                      flush=True)
                break
    print(f"{count} configurations, {bad} mismatches")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
