#!/usr/bin/env python3
"""Whole solver SESSIONS drawn at random, on the CPU: the product's host logic (csrc/mg_solver.c and its satellites, unchanged) over the
host-memory stand-ins of the kernel ABI, one Solver configuration and a sequence of operations on the same LIVE handle, every result compared
with a reference that knows nothing of what the handle did before.  What it can find is what the host layer decides between operations: which
buffer is u, whether the recorded coarse-level graph is still valid, what guess_nonzero, pre_done, jz_ready, last_sweep_pending, spec_valid and
iterate_behind mean after the previous operation.  tools/stress_solver_mock.py draws configurations; this draws what is done with them.
usage: stress_sessions_mock.py [count] [seed] [point|line] [only]        (only: run session number `only` of that count alone)

point   tests/mock_mgk_fmg.cpp + mg_solver.c + mg_comm.c + mg_fmg.c + mg_gmres.c.  dim, npts, levels (2 .. full depth), v0 in 1..5, v1 in 1..4,
        four damping factors, fuse (named sets and random values up to 65535: bits 14 and 15 toggle), pair_min_n, graph on / off.  One to four
        legs, each after a reset, a new right-hand side (manufactured | tests/rhs_cases.py uniform | spikes) or -- the FMG and GMRES legs, which
        never read the old iterate -- nothing at all:  solve | cycles(k1)[+cycles(k2)] + sync | fmg(nu)[+cycles(k)] | solve_fmg(nu) |
        solve_gmres(restart), which a reset + solve always follows.  References: Oracle.vcycle(fixed_cycles=, b=), tests/fmg_reference.py,
        tests/gmres_reference.py under the bars of tests/test_gmres_cpu.py (gmres_reference.judge).  GMRES legs are drawn where the hierarchy
        goes down to 3 x 3 or 1 x 1 and the reference converges fast enough for those bars (PointRef.gmres_can_be_judged says why); where it
        does not, the leg is drawn as solve_fmg(1).
line    tests/mock_mgk_xchunkline.cpp + mg_solver.c + mg_comm.c + mg_line.c + mg_xline.c + mg_line_chunk.c + mg_xline_chunk.c (and mg_fmg.c +
        mg_gmres.c over their stand-ins, tests/mock_mgk_sessions_line.cpp: the entry points that must refuse have to exist).  pc_type yline /
        xline / altline, npts, levels (1 .. full depth), v0 in 0..5, v1 in 1..4, meshes 0 / 1 / 2, the damping factors, line_chunk from
        {0, 2, 3, 5, 7, 8, 15, 16, 31, 63} and xline_chunk from {0, 16, 32, 48, 64} where the smoother takes them (periods with n = K c on some
        level, periods longer than every level), fuse, graph.  Legs: solve | cycles(k1)[+cycles(k2)] + sync after a reset or a new right-hand
        side.  One session in ten also calls fmg, solve_fmg or solve_gmres before a leg: MgError with the documented text, and the leg that
        follows still matches.  References: tests/xchunkline_reference.py / chunkline_reference.py Hierarchy with line_reference.solve (k fixed
        cycles: rtol=0.0, maxiter=k); hierarchies are cached per configuration.

After every leg: iterations equal, u bit-identical (np.array_equal), len(rnorm) == iterations + 1, ||b|| to 1e-12 and every entry of the history
to 1e-10 relative to ITSELF (tools/stress_solver_mock.py's rule; not to rnorm[0]: some drawn line configurations diverge -- xline on mesh 1
with scale 0.5 and one pre-sweep -- and stay in the draw, a wrong buffer shows fastest there).  A leg that runs to the tolerance takes a
right-hand side on which the REFERENCE's stop decision is clear of rounding (rhs_cases.stop_rule_clear: no norm within (1 +- 1e-6) rtol ||b||,
four decades wider than the agreement asked of the history; GMRES: the margins of gmres_reference.judge); another seed, of the other
family in turn, is drawn until it is; the manufactured one is replaced likewise.  Nothing is skipped: a session the solver refuses (other than the deliberate refusals) is a
failure.  Last line: `N sessions, M mismatches, R refused`; exit status 1 unless M = R = 0.  Every failure prints the solver keywords and the
operations as they ran, and `only` runs that session by itself.  Test infrastructure: the mock library is injected into the package's loader
cache HERE; the product has no such switch."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
RTOL, MAXITER = 1.0e-7, 40
SCALES = [0.8, 1.0, 6.0 / 7.0, 0.5]
LINE_CHUNKS = [0, 2, 3, 5, 7, 8, 15, 16, 31, 63]
XLINE_CHUNKS = [0, 16, 32, 48, 64]
SOURCES = {"point": ("mock_mgk_fmg.cpp", ("mg_solver.c", "mg_comm.c", "mg_fmg.c", "mg_gmres.c")),
           "line": ("mock_mgk_sessions_line.cpp", ("mg_solver.c", "mg_comm.c", "mg_line.c", "mg_xline.c", "mg_line_chunk.c", "mg_xline_chunk.c", "mg_fmg.c", "mg_gmres.c"))}
REFUSAL = {"yline": "built for point Jacobi (not the y-line smoother)", "xline": "built for point Jacobi (not the x-line or alternating line smoothers)",
           "altline": "built for point Jacobi (not the x-line or alternating line smoothers)"}


def build_mock(kind):
    """the mock-backed library of one kind under tests/_san/; built again only when a source is newer than it"""
    out = os.path.join(ROOT, "tests", "_san")
    os.makedirs(out, exist_ok=True)
    mock, host = SOURCES[kind]
    so = os.path.join(out, f"libmgsolve_sessions_{kind}.so")
    deps = [os.path.join(ROOT, "tests", f) for f in os.listdir(os.path.join(ROOT, "tests")) if f.startswith("mock_mgk")]
    deps += [os.path.join(d, f) for d in (CSRC, os.path.join(ROOT, "include")) for f in os.listdir(d) if f.endswith((".c", ".h"))]
    if os.path.exists(so) and os.path.getmtime(so) > max(os.path.getmtime(f) for f in deps):
        return so
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src in [os.path.join(ROOT, "tests", mock)] + [os.path.join(CSRC, f) for f in host]:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"sessions_{kind}_{os.path.basename(src)}.o")
        subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O2", "-fPIC", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L"] + inc +
                       ["-c", src, "-o", o], check=True)
        objs.append(o)
    subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread", "-ldl"], check=True)
    return so


def inject(kind):
    """build the mock-backed library and make the package's loader hand it out (before multigrid_petsc_amd.solver is imported)"""
    import multigrid_petsc_amd._lib as loader
    lib = ctypes.CDLL(build_mock(kind), mode=ctypes.RTLD_GLOBAL)
    loader._cache["mgk"] = lib
    loader._cache["mgpetsc"] = lib


def op_text(op):
    name, args = op[0], op[1:]
    if name == "cycles":
        return f"cycles({args[0]})" + (f" cycles({args[1]})" if args[1] else "") + " sync"
    if name == "fmg":
        return f"fmg({args[0]})" + (f" cycles({args[1]})" if args[1] else "")
    return f"{name}({', '.join(str(a) for a in args)})"


def runs_to_tolerance(op):
    return op[0] in ("solve", "solve_fmg", "solve_gmres")


# ----------------------------------------------------------------------------------------------------------------------------------
# the two draws: (solver keywords, legs); a leg is {"prep": None | "reset" | "rhs", "op": (name, args..), "refuse": None | name}
# ----------------------------------------------------------------------------------------------------------------------------------
def draw_point(rng, mock):
    dim = int(rng.choice([2, 3]))
    if mock:
        npts = int(rng.choice([9, 17, 33, 65, 129] if dim == 2 else [9, 17, 33]))
    else:
        npts = int(rng.choice([9, 17, 33, 65, 129, 257, 513, 1025] if dim == 2 else [9, 17, 33, 65, 129]))
    lmax = int(np.log2(npts - 1))
    levels = int(rng.integers(2, lmax + 1))
    v0, v1 = int(rng.integers(1, 6)), int(rng.integers(1, 5))
    scale = float(rng.choice(SCALES))
    no_tail = 63 | 256 | 1024 | 2048 | 4096 | 8192 | 16384
    fuse = int(rng.choice([-1, -1, 0, 32, 63, 63 | 256 | 512, no_tail, no_tail, no_tail & ~2, no_tail & ~8192, 63 | 256 | 512 | 1024 | 2048, 63 | 256 | 512 | 8192,
                           int(rng.integers(0, 65536)), int(rng.integers(0, 65536)), int(rng.integers(0, 65536)) | 32, int(rng.integers(0, 65536)) & ~512]))
    kw = dict(dim=dim, npts=npts, levels=levels, v=(v0, v1), maxiter=MAXITER, scale=scale, fuse=fuse, pair_min_n=int(rng.choice([0, 7, 7, 15, 31])),
              graph=int(rng.choice([-1, -1, 0])))
    kinds = ["solve", "cycles", "fmg", "fmg", "solve_fmg"] + (["solve_gmres"] if levels >= lmax - 1 else [])
    legs, nlegs = [], int(rng.integers(1, 5))
    while len(legs) < nlegs:
        name = str(rng.choice(kinds))
        if name == "solve":
            op, preps = ("solve",), ["reset", "rhs"]
        elif name == "cycles":
            op, preps = ("cycles", int(rng.integers(1, 5)), int(rng.integers(0, 4))), ["reset", "rhs"]
        elif name == "fmg":
            op, preps = ("fmg", int(rng.integers(1, 3)), int(rng.integers(0, 4))), [None, "reset", "rhs"]
        elif name == "solve_fmg":
            op, preps = ("solve_fmg", int(rng.integers(1, 3))), [None, "reset", "rhs"]
        else:
            op, preps = ("solve_gmres", int(rng.choice([3, 5, 10, 30]))), [None, "reset", "rhs"]
        legs.append(dict(prep="rhs" if not legs else preps[int(rng.integers(0, len(preps)))], op=op, refuse=None))
        if name == "solve_gmres":                         # a plain solve after it: a fresh solver's bits
            legs.append(dict(prep="reset", op=("solve",), refuse=None))
    return kw, legs


def draw_line(rng, mock):
    pc = str(rng.choice(["yline", "xline", "altline"]))
    npts = int(rng.choice([9, 17, 33, 65] if mock else [9, 17, 33, 65, 129, 257]))
    lmax = int(np.log2(npts - 1))
    levels = int(rng.integers(1, lmax + 1))
    v0, v1 = int(rng.integers(0, 6)), int(rng.integers(1, 5))
    if v0 == 0 and levels > 1:
        v0 = 1
    kw = dict(dim=2, npts=npts, levels=levels, v=(v0, v1), maxiter=MAXITER, scale=float(rng.choice(SCALES)), mesh=int(rng.choice([0, 1, 2])), pc_type=pc,
              line_chunk=int(rng.choice(LINE_CHUNKS)) if pc in ("yline", "altline") else 0, xline_chunk=int(rng.choice(XLINE_CHUNKS)) if pc in ("xline", "altline") else 0,
              fuse=int(rng.choice([-1, 0, int(rng.integers(0, 65536)), int(rng.integers(0, 65536))])), graph=int(rng.choice([-1, -1, 0])))
    legs = []
    for q in range(int(rng.integers(1, 4))):
        op = ("solve",) if rng.integers(0, 2) else ("cycles", int(rng.integers(1, 5)), int(rng.integers(0, 4)))
        legs.append(dict(prep="rhs" if q == 0 else str(rng.choice(["reset", "rhs"])), op=op, refuse=None))
    if rng.integers(0, 10) == 0:
        legs[int(rng.integers(0, len(legs)))]["refuse"] = str(rng.choice(["fmg", "solve_fmg", "solve_gmres"]))
    return kw, legs


# ----------------------------------------------------------------------------------------------------------------------------------
# the references: run(op, b) -> what the leg must give on the right-hand side b (None: the manufactured one), from a fresh start
# ----------------------------------------------------------------------------------------------------------------------------------
class PointRef:
    def __init__(self, orc, kw):
        self.orc, self.kw = orc, kw

    def run(self, op, b):
        import gmres_reference as G
        from fmg_reference import FmgRef
        kw, (v0, v1) = self.kw, self.kw["v"]
        if op[0] in ("solve", "cycles"):
            fixed = 0 if op[0] == "solve" else op[1] + op[2]
            kb = {} if b is None else dict(b=b)
            return self.orc.vcycle(kw["dim"], kw["npts"], kw["levels"], v0, v1, maxiter=max(MAXITER, fixed), scale=kw["scale"], fixed_cycles=fixed, **kb)
        if op[0] in ("fmg", "solve_fmg"):
            f = FmgRef(self.orc, kw["dim"], kw["npts"], kw["levels"], (v0, v1), kw["scale"], b0=b)
            if op[0] == "fmg":
                u, rn = f.fmg_then_cycles(op[1], op[2])
                return {"iters": op[2] + 1, "u": u, "rnorm": rn, "bnorm": f.bnorm()}
            it, u, rn = f.solve_fmg(op[1], maxiter=MAXITER, rtol=RTOL)
            return {"iters": it, "u": u, "rnorm": rn, "bnorm": f.bnorm()}
        ops = G.Operators(self.orc, kw["dim"], kw["npts"], kw["levels"], 0, kw["scale"], v=(v0, v1))
        bb = ops.rhs() if b is None else b
        refs = [G.gmres(ops, bb, op[1], rtol=RTOL, maxiter=MAXITER, dot=d) for d in ("np", "ld")]
        ops.close()
        return {"refs": refs, "b": bb}

    def clear(self, op, ref):
        import gmres_reference as G
        import rhs_cases
        if op[0] != "solve_gmres":
            return rhs_cases.stop_rule_clear(ref, RTOL)
        m = [G.margins(r, RTOL) for r in ref["refs"]]
        return ref["refs"][0]["iters"] == ref["refs"][1]["iters"] and all(last <= 0.8 and before >= 1.5 for last, before in m)

    def gmres_can_be_judged(self, op, rng):
        """gmres_reference.judge asks for a converged solve whose last estimate is <= 0.8 and the one before >= 1.5 rtol ||b||.  Where the
        GMRES history ends relative to rtol ||b|| is a property of the cycle and the restart length far more than of the right-hand side
        (measured: uniform and spike fields of one size end within a few per cent of each other), so another seed does not move a history off
        the threshold.  Decided on the REFERENCE alone, on a uniform right-hand side: it converges within the count and ends at <= 0.7 after
        >= 1.8 -- inside those margins with room for the few per cent.  Elsewhere the leg is drawn as solve_fmg(1)"""
        import gmres_reference as G
        import rhs_cases
        r = self.run(op, rhs_cases.uniform(self.kw["dim"], self.kw["npts"], int(rng.integers(1 << 30))))["refs"][1]
        last, before = G.margins(r, RTOL)
        return r["iters"] < MAXITER and last <= 0.7 and before >= 1.8

    def gmres_agrees(self, ref, it, u, rn, bn):
        import gmres_reference as G
        kw = self.kw
        try:
            G.judge(self.orc, (kw["dim"], kw["npts"], kw["levels"], 0, kw["scale"]), ref["b"], ref["refs"], it, rn, u, bn, RTOL)
        except AssertionError as e:
            return f"gmres_reference.judge: {e!r}"
        return None


class LineRef:
    _cache = {}

    def __init__(self, orc, kw):
        import chunkline_reference as CR
        import xchunkline_reference as XC
        key = (kw["pc_type"], kw["npts"], kw["levels"], kw["mesh"], kw["xline_chunk"], kw["line_chunk"])
        if key not in LineRef._cache:
            if len(LineRef._cache) > 400:
                LineRef._cache.clear()
            LineRef._cache[key] = (CR.Hierarchy(orc, kw["npts"], kw["levels"], kw["mesh"], kw["line_chunk"]) if kw["pc_type"] == "yline" else
                                   XC.Hierarchy(orc, kw["npts"], kw["levels"], kw["mesh"], kw["pc_type"], kw["xline_chunk"], kw["line_chunk"]))
        self.h, self.kw = LineRef._cache[key], kw

    def run(self, op, b):
        import line_reference as LR
        bb = self.h.rhs() if b is None else b
        if op[0] == "solve":
            return LR.solve(self.h, bb, self.kw["scale"], v=self.kw["v"], rtol=RTOL, maxiter=MAXITER)
        return LR.solve(self.h, bb, self.kw["scale"], v=self.kw["v"], rtol=0.0, maxiter=op[1] + op[2])

    def clear(self, op, ref):
        import rhs_cases
        return rhs_cases.stop_rule_clear(ref, RTOL)


def agrees(ref, it, u, rn, bn):
    """the comparison rules; None, or what differs"""
    if it != ref["iters"]:
        return f"iterations {it}, reference {ref['iters']}"
    if len(rn) != it + 1 or len(rn) != len(ref["rnorm"]):
        return f"len(rnorm) {len(rn)}, iterations {it}, reference {len(ref['rnorm'])}"
    if not np.array_equal(u, ref["u"]):
        return f"u differs: max|du| {float(np.max(np.abs(u - ref['u']))):.3e} at {int(np.count_nonzero(u != ref['u']))} of {u.size} points"
    if not abs(bn - ref["bnorm"]) <= 1e-12 * ref["bnorm"]:
        return f"bnorm {bn!r}, reference {ref['bnorm']!r}"
    d = float(np.max(np.abs(rn - ref["rnorm"]) / np.maximum(ref["rnorm"], 1e-300)))
    if not d <= 1e-10:
        return f"rnorm differs by {d:.3e} relative"
    return None


# ----------------------------------------------------------------------------------------------------------------------------------
# one session
# ----------------------------------------------------------------------------------------------------------------------------------
def plan_right_hand_sides(rng, R, kw, legs):
    """the right-hand side of every "rhs" step -- (kind, seed, b), b None for the manufactured one -- and every leg's reference on the one it
    runs on.  A leg that runs to the tolerance needs a clear stop decision on the reference: another seed until every such leg of the segment
    has one"""
    import rhs_cases
    dim, npts = kw["dim"], kw["npts"]
    start = [q for q, leg in enumerate(legs) if leg["prep"] == "rhs"]
    for a, z in zip(start, start[1:] + [len(legs)]):
        kind = str(rng.choice(["uniform", "spikes", "problem"], p=[0.4, 0.4, 0.2]))
        if kind == "spikes" and npts < rhs_cases.spikes_min_npts(dim):
            kind = "uniform"
        for attempt in range(60):
            seed = int(rng.integers(1 << 30))
            b = None if kind == "problem" else rhs_cases.make(kind, dim, npts, seed)
            refs = []
            for leg in legs[a:z]:
                refs.append(R.run(leg["op"], b))
                if runs_to_tolerance(leg["op"]) and not R.clear(leg["op"], refs[-1]):
                    break
            else:
                break
            # the manufactured one has nothing to redraw; uniform fields of one size all give nearly the same history relative to ||b||, a
            # handful of spikes does not: the families take turns where the grid has room for spikes
            kind = "spikes" if kind != "spikes" and npts >= rhs_cases.spikes_min_npts(dim) else "uniform"
        else:
            raise RuntimeError(f"no right-hand side with a clear stop decision in 60 draws for the legs {a} .. {z - 1}")
        for leg, ref in zip(legs[a:z], refs):
            leg["ref"] = ref
        legs[a]["rhs"] = (kind, None if kind == "problem" else seed, b)


def run_session(rng, orc, kind, kw, legs, tag):
    """(mismatches, refusals) of one session: 1, 0 | 0, 1 | 0, 0"""
    from multigrid_petsc_amd.solver import MgError, Solver
    done = []

    def report(what, why):
        print(what, tag, f"Solver(**{kw!r})", "operations:", "; ".join(done), "--", why, flush=True)

    R = (PointRef if kind == "point" else LineRef)(orc, kw)
    for leg in legs:
        if leg["op"][0] == "solve_gmres" and not R.gmres_can_be_judged(leg["op"], rng):
            leg["op"] = ("solve_fmg", 1)
    try:
        plan_right_hand_sides(rng, R, kw, legs)
    except RuntimeError as e:                                # (counted with the refusals: the draw is to produce sessions that can be judged)
        report("REFUSED", f"{e}; legs: {'; '.join(op_text(leg['op']) for leg in legs)}")
        return 0, 1

    s = None
    try:
        s = Solver(**kw)
        done.append("create")
        for leg in legs:
            op = leg["op"]
            if leg["prep"] == "rhs":
                rk, seed, b = leg["rhs"]
                done.append("set_rhs_problem()" if b is None else f"set_rhs(rhs_cases.make({rk!r}, {kw['dim']}, {kw['npts']}, {seed}))")
                s.set_rhs_problem() if b is None else s.set_rhs(b)
            elif leg["prep"] == "reset":
                done.append("reset()")
                s.reset()
            if leg["refuse"]:
                done.append(f"{leg['refuse']}: must be refused")
                try:
                    getattr(s, leg["refuse"])(*((5,) if leg["refuse"] == "solve_gmres" else (1,)))
                    report("MISMATCH", f"{leg['refuse']} was accepted with pc_type {kw['pc_type']}")
                    return 1, 0
                except MgError as e:
                    if REFUSAL[kw["pc_type"]] not in str(e):
                        report("MISMATCH", f"refused with another text: {e}")
                        return 1, 0
            done.append(op_text(op))
            if op[0] == "cycles":
                s.cycles(op[1])
                if op[2]:
                    s.cycles(op[2])
                s.sync()
            elif op[0] == "fmg":
                s.fmg(op[1])
                if op[2]:
                    s.cycles(op[2])
                    s.sync()
            else:
                getattr(s, op[0])(*op[1:])
            it, u, rn, bn = s.iterations, s.solution(), s.rnorm, s.bnorm
            why = R.gmres_agrees(leg["ref"], it, u, rn, bn) if op[0] == "solve_gmres" else agrees(leg["ref"], it, u, rn, bn)
            if why:
                report("MISMATCH", why)
                return 1, 0
        return 0, 0
    except MgError as e:
        report("REFUSED", str(e)[:200])
        return 0, 1
    finally:
        if s is not None:
            s.close()


def main(mock=True):
    """mock=False: the same draws on the GPU over the real libraries, with the larger sizes (tools/stress_sessions.py)"""
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    kind = sys.argv[3] if len(sys.argv) > 3 else "point"
    only = int(sys.argv[4]) if len(sys.argv) > 4 else None
    if kind not in SOURCES:
        sys.exit(f"session kind {kind!r}: point or line")
    if mock:
        inject(kind)
    from oracle import Oracle
    orc = Oracle()
    bad = refused = 0
    tally = {}
    for q in range(count) if only is None else [only]:
        rng = np.random.default_rng([seed, q, 0 if kind == "point" else 1])        # a generator of its own: session q runs alone as it runs in the row
        kw, legs = (draw_point if kind == "point" else draw_line)(rng, mock)
        m, r = run_session(rng, orc, kind, kw, legs, f"session {q} of `{count} {seed} {kind}`:")
        bad, refused = bad + m, refused + r
        for leg in legs:
            for name in [leg["op"][0]] + (["refusals"] if leg["refuse"] else []) + (["new right-hand sides"] if leg["prep"] == "rhs" else []):
                tally[name] = tally.get(name, 0) + 1
    print("legs drawn:", ", ".join(f"{k} {v}" for k, v in sorted(tally.items())))
    print(f"{count if only is None else 1} sessions, {bad} mismatches, {refused} refused")
    sys.exit(1 if bad or refused else 0)


if __name__ == "__main__":
    main()
