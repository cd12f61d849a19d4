"""Worker of tests/test_cheby_fused_cpu.py: the product's Solver over a shared library that holds mg_solver.c, mg_comm.c, mg_cheby.c and the
host-memory stand-ins (tests/mock_mgk_cheby.cpp) in place of libmgk.so / libmgpetsc.so.  A process of its own, because the loader caches
the libraries it hands out.  argv: library, output .npz, then one 'dim,npts,levels,mesh' per case."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EIG = (0.2, 2.0)
NCYC = 5


def main():
    so, out = sys.argv[1], sys.argv[2]
    import multigrid_petsc_amd._lib as loader
    lib = ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)
    loader._cache["mgk"] = lib
    loader._cache["mgpetsc"] = lib
    from multigrid_petsc_amd.solver import Solver
    lib.mock_cheby_calls.restype = ctypes.c_int
    lib.mock_cheby_calls.argtypes = [ctypes.c_int]
    calls = lambda: np.array([lib.mock_cheby_calls(q) for q in range(5)])
    res = {}
    for case in sys.argv[3:]:
        dim, npts, levels, mesh = (int(x) for x in case.split(","))
        for tag, fuse in (("on", -1), ("off", (63 | 0xFF00) & ~32768)):
            s = Solver(dim, npts, levels, v=(3, 3), maxiter=60, ksp_type="chebyshev", eigenvalues=EIG, fuse=fuse, mesh=mesh)
            s.set_rhs_problem()
            lib.mock_cheby_calls_reset()
            it = s.solve()
            k = f"{case}:{tag}:"
            res[k + "it"], res[k + "rn"], res[k + "u"], res[k + "calls"] = it, s.rnorm, s.solution(), calls()
            lib.mock_cheby_calls_reset()
            s.reset()
            s.cycles(NCYC)
            s.sync()
            res[k + "rn5"], res[k + "u5"], res[k + "calls5"] = s.rnorm, s.solution(), calls()
            # a solve after the fixed run: the recorded graph is replayed from fresh state
            s.reset()
            assert s.solve() == it and np.array_equal(s.solution(), res[k + "u"])
            s.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
