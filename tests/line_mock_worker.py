"""Worker of tests/test_line_cpu.py: the product's Solver over a shared library that holds mg_solver.c, mg_comm.c, mg_line.c and the
host-memory stand-ins (tests/mock_mgk_line.cpp) in place of libmgk.so / libmgpetsc.so.  A process of its own, because the loader caches
the libraries it hands out.  argv: library, output .npz, then one 'npts,levels,mesh,rhs' per case (rhs: 'manufactured' or 'rough:<seed>',
tests/rhs_cases.uniform).  Every case: Solver(pc_type="yline", scale=0.8) with the defaults, with graph=0, with fuse=0, and reset + solve."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
SCALE = 0.8


def main():
    so, out = sys.argv[1], sys.argv[2]
    import multigrid_petsc_amd._lib as loader
    lib = ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)
    loader._cache["mgk"] = lib
    loader._cache["mgpetsc"] = lib
    import rhs_cases
    from multigrid_petsc_amd.solver import MgError, Solver
    lib.mock_line_calls.restype = ctypes.c_int
    lib.mock_line_calls.argtypes = [ctypes.c_int]
    res = {}
    for case in sys.argv[3:]:
        f = case.split(",")
        npts, levels, mesh, rhs = int(f[0]), int(f[1]), int(f[2]), f[3]

        def make(**kw):
            s = Solver(2, npts, levels, v=(3, 3), maxiter=100, scale=SCALE, mesh=mesh, pc_type="yline", **kw)
            if rhs == "manufactured":
                s.set_rhs_problem()
            else:
                s.set_rhs(rhs_cases.uniform(2, npts, int(rhs.split(":")[1])))
            return s

        k = case + ":"
        s = make()
        lib.mock_line_calls_reset()
        it = s.solve()
        res[k + "it"], res[k + "rn"], res[k + "u"], res[k + "bnorm"] = it, s.rnorm, s.solution(), s.bnorm
        res[k + "calls"] = np.array([lib.mock_line_calls(0), lib.mock_line_calls(1)])
        s.reset()
        assert s.solve() == it and np.array_equal(s.rnorm, res[k + "rn"]) and np.array_equal(s.solution(), res[k + "u"]), "reset + solve differs"
        s.close()
        for tag, kw in (("graph0", dict(graph=0)), ("fuse0", dict(fuse=0))):
            s = make(**kw)
            res[k + tag + "_it"], res[k + tag + "_rn"], res[k + tag + "_u"] = s.solve(), s.rnorm, s.solution()
            s.close()
    # what the line smoother is not built for is refused at creation, with the reason
    for kw, msg in ((dict(dim=3, npts=17, levels=3), "built for 2-D"),
                    (dict(dim=2, npts=17, levels=3, precision="mixed"), "not mixed precision"),
                    (dict(dim=2, npts=17, levels=3, ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev"),
                    (dict(dim=2, npts=17, levels=3, nranks=2), "one GPU")):
        try:
            Solver(v=(3, 3), maxiter=20, scale=SCALE, pc_type="yline", **kw)
            raise SystemExit(f"{kw} was accepted")
        except MgError as e:
            assert msg in str(e) and "y-line" in str(e), str(e)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
