"""Worker of tests/test_line_tail_cpu.py: the product's Solver over a shared library that holds mg_solver.c, mg_comm.c, mg_line.c, mg_xline.c,
mg_line_tail.c and the host-memory stand-ins (tests/mock_mgk_line_tail.cpp) in place of libmgk.so / libmgpetsc.so.  A process of its own,
because the loader caches the libraries it hands out.  argv: library, output .npz, then one 'pc,npts,levels,mesh,rhs' per case (rhs:
'manufactured' or 'rough:<seed>', tests/rhs_cases.uniform).  Every case: Solver(pc_type=pc, scale=0.8, line_tail=1) with the log of line
passes and tail calls, reset + solve, the same with line_tail=0, with graph=0 and with fuse=0.  Then v = (2, 1) and (1, 2) on a small case,
the fall-backs and the refusals.  "--without-mg-line-tail" instead of the cases: only what a library linked without mg_line_tail.c must do."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
SCALE = 0.8
ORDER = ("altline", 33, 5, 2, "manufactured")


def main():
    so, out = sys.argv[1], sys.argv[2]
    import multigrid_petsc_amd._lib as loader
    lib = ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)
    loader._cache["mgk"] = lib
    loader._cache["mgpetsc"] = lib
    import rhs_cases
    from multigrid_petsc_amd.solver import MgError, Solver

    def make(pc, npts, levels, mesh, rhs, v=(3, 3), **kw):
        s = Solver(2, npts, levels, v=v, maxiter=100, scale=SCALE, mesh=mesh, pc_type=pc, **kw)
        if rhs == "manufactured":
            s.set_rhs_problem()
        else:
            s.set_rhs(rhs_cases.uniform(2, npts, int(rhs.split(":")[1])))
        return s

    if sys.argv[3:] == ["--without-mg-line-tail"]:
        # a library linked without mg_line_tail.c (the x-line tier's link): line_tail = 1 is refused with a message, line_tail = 0 runs as before
        for pc in ("yline", "xline", "altline"):
            try:
                Solver(2, 33, 5, scale=SCALE, pc_type=pc, line_tail=1)
                raise SystemExit(f"{pc} with line_tail=1 was accepted")
            except MgError as e:
                assert "mg_line_tail.c is not linked" in str(e), str(e)
        s = make(*ORDER, line_tail=0)
        np.savez(out, it=s.solve(), rn=s.rnorm, u=s.solution(), tail_level=s.tail_level)
        s.close()
        return
    lib.mock_xline_log.restype = ctypes.c_char_p
    res = {}
    for case in sys.argv[3:]:
        f = case.split(",")
        pc, npts, levels, mesh, rhs = f[0], int(f[1]), int(f[2]), int(f[3]), f[4]
        k = case + ":"
        s = make(pc, npts, levels, mesh, rhs, line_tail=1)
        lib.mock_xline_log_clear()
        it = s.solve()
        res[k + "it"], res[k + "rn"], res[k + "u"], res[k + "bnorm"] = it, s.rnorm, s.solution(), s.bnorm
        res[k + "log"] = lib.mock_xline_log().decode()
        res[k + "tail_level"], res[k + "dof"] = s.tail_level, s.dof_updates_per_cycle
        s.reset()
        assert s.solve() == it and np.array_equal(s.rnorm, res[k + "rn"]) and np.array_equal(s.solution(), res[k + "u"]), "reset + solve differs"
        s.close()
        for tag, kw in (("off", dict(line_tail=0)), ("graph0", dict(line_tail=1, graph=0)), ("fuse0", dict(line_tail=1, fuse=0))):
            s = make(pc, npts, levels, mesh, rhs, **kw)
            lib.mock_xline_log_clear()
            res[k + tag + "_it"], res[k + tag + "_rn"], res[k + tag + "_u"] = s.solve(), s.rnorm, s.solution()
            res[k + tag + "_log"] = lib.mock_xline_log().decode()
            res[k + tag + "_tail_level"], res[k + tag + "_dof"] = s.tail_level, s.dof_updates_per_cycle
            s.close()
    # other sweep counts: the tail's own count of v1 sweeps on the coarsest level and of v0 above it
    for v in ((2, 1), (1, 2)):
        for lt in (1, 0):
            s = make(*ORDER, v=v, line_tail=lt)
            lib.mock_xline_log_clear()
            k = f"v:{v[0]},{v[1]},{lt}:"
            res[k + "it"], res[k + "rn"], res[k + "u"] = s.solve(), s.rnorm, s.solution()
            res[k + "log"], res[k + "tail_level"] = lib.mock_xline_log().decode(), s.tail_level
            s.close()
    # accepted, and the tail stays off: fewer than two levels would be left (levels = 2 at 257), no pre-smoothing (v0 = 0)
    for tag, args, kw in (("two", ("altline", 257, 2, 0, "manufactured"), dict()), ("v0", ("altline", 33, 5, 1, "manufactured"), dict(v=(0, 3)))):
        kw = dict(kw)
        if tag == "v0":
            kw["maxiter"] = 3
        for lt in (1, 0):
            pc, npts, levels, mesh, rhs = args
            s = Solver(2, npts, levels, v=kw.get("v", (3, 3)), maxiter=kw.get("maxiter", 5), scale=SCALE, mesh=mesh, pc_type=pc, line_tail=lt)
            s.set_rhs_problem()
            k = f"fallback:{tag},{lt}:"
            res[k + "it"], res[k + "rn"], res[k + "u"], res[k + "tail_level"] = s.solve(), s.rnorm, s.solution(), s.tail_level
            s.close()
    # refusals
    for kw, msg in ((dict(pc_type="altline", line_tail=2), "line_tail must be 0 (off) or 1"),
                    (dict(pc_type="yline", line_tail=-1), "line_tail must be 0 (off) or 1"),
                    (dict(pc_type="jacobi", line_tail=1), "line_tail goes with the line smoothers")):
        try:
            Solver(2, 33, 5, scale=SCALE, **kw)
            raise SystemExit(f"{kw} was accepted")
        except MgError as e:
            assert msg in str(e), str(e)
    # point Jacobi's own tail (fuse bit 9) shows through the same accessor
    s = Solver(2, 33, 5, scale=SCALE)
    res["jacobi_tail_level"] = s.tail_level
    s.close()
    res["tail_calls"] = lib.mock_line_tail_calls()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
