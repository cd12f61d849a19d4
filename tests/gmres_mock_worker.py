"""Worker of tests/test_gmres_cpu.py: the product's Solver over a shared library that holds mg_solver.c, mg_comm.c, mg_gmres.c and the
host-memory stand-ins (tests/mock_mgk_gmres.cpp) in place of libmgk.so / libmgpetsc.so.  A process of its own, because the loader caches
the libraries it hands out.  argv: library, output .npz, then one 'dim,npts,levels,mesh,scale,restart,rhs,maxiter' per case
(rhs: 'manufactured' or 'rough:<seed>', tests/rhs_cases.uniform)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def main():
    so, out = sys.argv[1], sys.argv[2]
    import multigrid_petsc_amd._lib as loader
    lib = ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)
    loader._cache["mgk"] = lib
    loader._cache["mgpetsc"] = lib
    import rhs_cases
    from multigrid_petsc_amd.solver import MgError, Solver
    lib.mock_gmres_calls.restype = ctypes.c_int
    lib.mock_gmres_calls.argtypes = [ctypes.c_int]
    calls = lambda: np.array([lib.mock_gmres_calls(q) for q in range(5)])
    res = {}
    for case in sys.argv[3:]:
        f = case.split(",")
        dim, npts, levels, mesh, scale, restart, rhs, maxiter = int(f[0]), int(f[1]), int(f[2]), int(f[3]), float(f[4]), int(f[5]), f[6], int(f[7])

        def make():
            s = Solver(dim, npts, levels, v=(3, 3), maxiter=maxiter, scale=scale, mesh=mesh)
            if rhs == "manufactured":
                s.set_rhs_problem()
            else:
                s.set_rhs(rhs_cases.uniform(dim, npts, int(rhs.split(":")[1])))
            return s

        k = case + ":"
        fresh = make()
        res[k + "plain_it"], res[k + "plain_rn"], res[k + "plain_u"] = fresh.solve(), fresh.rnorm, fresh.solution()
        fresh.close()
        s = make()
        lib.mock_gmres_calls_reset()
        it = s.solve_gmres(restart)
        res[k + "it"], res[k + "rn"], res[k + "x"], res[k + "calls"], res[k + "bnorm"] = it, s.rnorm, s.solution(), calls(), s.bnorm
        # a second call and another (longer) basis on the same solver
        assert s.solve_gmres(restart) == it and np.array_equal(s.solution(), res[k + "x"]) and np.array_equal(s.rnorm, res[k + "rn"])
        it2 = s.solve_gmres(min(restart + 2, 32))
        res[k + "it_other_restart"] = it2
        # a plain solve afterwards: a fresh solver's history and field, bit for bit
        s.reset()
        res[k + "after_it"], res[k + "after_rn"], res[k + "after_u"] = s.solve(), s.rnorm, s.solution()
        for m in (0, 33):
            try:
                s.solve_gmres(m)
                raise SystemExit(f"restart {m} was accepted")
            except MgError as e:
                assert "restart must be within" in str(e), str(e)
        s.close()
    # refusals that need another configuration
    for kw, msg in ((dict(ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev"), (dict(precision="mixed"), "not mixed precision")):
        s = Solver(3, 17, 3, v=(3, 3), maxiter=20, scale=0.8, **kw)
        s.set_rhs_problem()
        try:
            s.solve_gmres(30)
            raise SystemExit(f"{kw} was accepted")
        except MgError as e:
            assert msg in str(e), str(e)
        s.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
