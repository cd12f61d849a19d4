"""Worker of tests/test_cg_mixed_cpu.py: the product's Solver (precision="mixed") over a shared library that holds mg_solver.c, mg_comm.c, mg_cg.c,
mg_cg_mixed.c, mg_gmres.c and the host-memory stand-ins (tests/mock_mgk_cg_mixed.cpp) in place of libmgk.so / libmgpetsc.so.  A process of its
own, because the loader caches the libraries it hands out.  argv: library, output .npz, then one case per argument in the spelling of
cg_reference.key."""
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
    import cg_mixed_reference as R
    import rhs_cases
    from multigrid_petsc_amd.solver import MgError, Solver
    for f in (lib.mock_cg_mixed_calls, lib.mock_cg_calls):
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int]
    lib.mock_cg_fail_malloc.argtypes = [ctypes.c_long]
    # dot, direction, update of the mixed passes; then the fp64 direction and update passes and mgk_multi_dot_f64, which must stay at 0
    calls = lambda: np.array([lib.mock_cg_mixed_calls(q) for q in range(3)] + [lib.mock_cg_calls(q) for q in range(3)])
    res = {}

    def make(case, b, precision="mixed", **kw):
        dim, npts, levels, scale, v, rhs, maxiter = case
        s = Solver(dim, npts, levels, v=v, maxiter=maxiter, scale=scale, precision=precision, **kw)
        s.set_rhs(b)
        return s

    for text in sys.argv[3:]:
        case = R.parse(text)
        k = text + ":"
        b = rhs_cases.uniform(3, case[1], int(case[5].split(":")[1]))
        fresh = make(case, b)
        res[k + "plain_it"], res[k + "plain_rn"], res[k + "plain_u"] = fresh.solve(), fresh.rnorm, fresh.solution()
        fresh.close()
        s = make(case, b)
        lib.mock_cg_mixed_calls_reset()
        it = s.solve_cg_mixed()
        res[k + "it"], res[k + "rn"], res[k + "x"], res[k + "calls"], res[k + "bnorm"], res[k + "breakdown"] = it, s.rnorm, s.solution(), calls(), s.bnorm, s.cg_breakdown
        # the same call again: the same bits
        assert s.solve_cg_mixed() == it and np.array_equal(s.solution(), res[k + "x"]) and np.array_equal(s.rnorm, res[k + "rn"])
        # a second right-hand side on the live handle: what a fresh solver makes of it, bit for bit
        b2 = rhs_cases.uniform(3, case[1], 77)
        s.set_rhs(b2)
        it2, rn2, x2 = s.solve_cg_mixed(), s.rnorm, s.solution()
        other = make(case, b2)
        assert other.solve_cg_mixed() == it2 and np.array_equal(other.rnorm, rn2) and np.array_equal(other.solution(), x2), "second right-hand side"
        other.close()
        res[k + "it_rhs2"] = it2
        # reset + a plain mixed solve afterwards: a fresh mixed solver's history and field, bit for bit (level 0's b is the caller's again)
        s.set_rhs(b)
        assert s.solve_cg_mixed() == it and np.array_equal(s.solution(), res[k + "x"])
        s.reset()
        res[k + "after_it"], res[k + "after_rn"], res[k + "after_u"] = s.solve(), s.rnorm, s.solution()
        s.close()
        # without the coarse-level graph and without any fused pass (no e0 from the update pass): the bits of the defaults
        if case == R.CASES[0]:
            for kw in (dict(graph=0), dict(fuse=0)):
                q = make(case, b, **kw)
                assert q.solve_cg_mixed() == it and np.array_equal(q.rnorm, res[k + "rn"]) and np.array_equal(q.solution(), res[k + "x"]), kw
                q.close()
    # the refusals a configuration reaches (the others need a handle that mg_solver_create does not make: tests/san_cg_mixed.c); the handle stays usable
    case = R.CASES[0]
    b = rhs_cases.uniform(3, 17, 3)
    s = Solver(3, 17, 3, v=(3, 3), maxiter=20, scale=0.8)
    s.set_rhs(b)
    try:
        s.solve_cg_mixed()
        raise SystemExit("an fp64 solver was accepted")
    except MgError as e:
        assert "mg_solver_solve_cg_mixed" in str(e) and "built for a mixed-precision solver" in str(e), str(e)
    assert s.cg_breakdown == 0 and s.solve_cg() >= 1
    s.close()
    s = Solver(3, 17, 3, v=(3, 3), maxiter=20, scale=0.8, precision="mixed")
    s.set_rhs(b)
    try:
        s.solve_cg()
        raise SystemExit("mg_solver_solve_cg took a mixed solver")
    except MgError as e:
        assert "not mixed precision" in str(e), str(e)
    # the five fields do not fit: the error names the count and the bytes, nothing stays allocated, and the next call succeeds
    lib.mock_cg_fail_malloc(3)
    try:
        s.solve_cg_mixed()
        raise SystemExit("the failed allocation went unnoticed")
    except MgError as e:
        assert "mg_solver_solve_cg_mixed: needs 5 fine-level fields of" in str(e) and "bytes" in str(e), str(e)
    assert lib.mock_cg_live_allocations() == 0
    res["alloc_retry_it"] = s.solve_cg_mixed()
    s.close()
    # no step: maxiter 0 and a zero right-hand side
    s = Solver(3, 17, 3, v=(3, 3), maxiter=0, scale=0.8, precision="mixed")
    s.set_rhs(b)
    assert s.solve_cg_mixed() == 0 and not s.solution().any() and s.cg_breakdown == 0
    s.close()
    s = Solver(3, 17, 3, v=(3, 3), maxiter=20, scale=0.8, precision="mixed")
    s.set_rhs(np.zeros(15 ** 3))
    assert s.solve_cg_mixed() == 0 and not s.solution().any() and s.bnorm == 0.0
    s.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
