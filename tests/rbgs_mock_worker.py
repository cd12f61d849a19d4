"""Worker of tests/test_rbgs_cpu.py: the product's Solver over a shared library that holds mg_solver.c, mg_comm.c, mg_rbgs.c, mg_fmg.c, mg_gmres.c
and the host-memory stand-ins (tests/mock_mgk_rbgs.cpp) in place of libmgk.so / libmgpetsc.so.  A process of its own, because the loader
caches the libraries it hands out.  argv: library, output .npz, then one 'npts,mesh,scale,v0,v1,rhs' per case (tests/rbgs_reference.py; levels
down to 1 x 1).  Every case: Solver(pc_type="rbgs") with the defaults, with graph=0, with fuse=0; a second right-hand side on the live handle;
reset + solve; the stand-ins' execution counts.  Then every refusal, by its message, and a handle that stays usable after a refused fmg."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
SECOND_RHS_SEED = 3


def main():
    so, out = sys.argv[1], sys.argv[2]
    import multigrid_petsc_amd._lib as loader
    lib = ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)
    loader._cache["mgk"] = lib
    loader._cache["mgpetsc"] = lib
    import rhs_cases
    from rbgs_reference import LEVELS
    from multigrid_petsc_amd.solver import MgError, Solver
    lib.mock_rbgs_calls.restype = ctypes.c_int
    lib.mock_rbgs_calls.argtypes = [ctypes.c_int]
    res = {}
    for case in sys.argv[3:]:
        f = case.split(",")
        npts, mesh, scale, v0, v1, rhs = int(f[0]), int(f[1]), float(f[2]), int(f[3]), int(f[4]), f[5]
        assert rhs == "manufactured"

        def make(**kw):
            s = Solver(2, npts, LEVELS[npts], v=(v0, v1), maxiter=100, scale=scale, mesh=mesh, pc_type="rbgs", **kw)
            s.set_rhs_problem()
            return s

        k = case + ":"
        s = make()
        lib.mock_rbgs_calls_reset()
        it = s.solve()
        res[k + "it"], res[k + "rn"], res[k + "u"], res[k + "bnorm"] = it, s.rnorm, s.solution(), s.bnorm
        res[k + "calls"] = np.array([lib.mock_rbgs_calls(q) for q in range(3)])
        res[k + "dof"] = s.dof_updates_per_cycle
        # a second right-hand side on the live handle, then the first one again: reset + solve repeats the first solve
        s.set_rhs(rhs_cases.uniform(2, npts, SECOND_RHS_SEED))
        s.reset()
        res[k + "second_it"], res[k + "second_rn"], res[k + "second_u"], res[k + "second_bnorm"] = s.solve(), s.rnorm, s.solution(), s.bnorm
        s.set_rhs_problem()
        s.reset()
        assert s.solve() == it and np.array_equal(s.rnorm, res[k + "rn"]) and np.array_equal(s.solution(), res[k + "u"]), "reset + solve differs"
        s.close()
        for tag, kw in (("graph0", dict(graph=0)), ("fuse0", dict(fuse=0))):
            s = make(**kw)
            res[k + tag + "_it"], res[k + tag + "_rn"], res[k + tag + "_u"] = s.solve(), s.rnorm, s.solution()
            s.close()
    # what the smoother is not built for is refused at creation, with the reason
    for kw, msg in ((dict(dim=3, npts=17, levels=3), "built for 2-D"),
                    (dict(dim=2, npts=17, levels=3, precision="mixed"), "not mixed precision"),
                    (dict(dim=2, npts=17, levels=3, ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev"),
                    (dict(dim=2, npts=17, levels=3, nranks=2), "one GPU"),
                    (dict(dim=2, npts=17, levels=3, line_chunk=4), "must be 0 with pc_type rbgs"),
                    (dict(dim=2, npts=33, levels=3, xline_chunk=16), "must be 0 with pc_type rbgs"),
                    (dict(dim=2, npts=17, levels=3, line_tail=1), "must be 0 with pc_type rbgs")):
        try:
            Solver(v=(2, 2), maxiter=20, scale=1.0, pc_type="rbgs", **kw)
            raise SystemExit(f"{kw} was accepted")
        except MgError as e:
            assert msg in str(e) and ("red-black Gauss-Seidel" in str(e) or "rbgs" in str(e)), str(e)
    # fmg, solve_fmg and solve_gmres on such a solver: each refused with a message of its own; the handle is still usable afterwards
    s = Solver(2, 17, 4, v=(2, 2), maxiter=100, scale=1.0, pc_type="rbgs")
    s.set_rhs_problem()
    it = s.solve()
    u = s.solution()
    for call, name in ((lambda: s.fmg(1), "mg_solver_fmg"), (lambda: s.solve_fmg(1), "mg_solver_fmg"), (lambda: s.solve_gmres(5), "mg_solver_solve_gmres")):
        try:
            call()
            raise SystemExit(f"{name} was accepted")
        except MgError as e:
            assert name in str(e) and "not the red-black Gauss-Seidel smoother" in str(e), str(e)
        s.reset()
        assert s.solve() == it and np.array_equal(s.solution(), u), f"the handle is not usable after a refused {name}"
    s.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
