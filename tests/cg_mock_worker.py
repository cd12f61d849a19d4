"""Worker of tests/test_cg_cpu.py: the product's Solver over a shared library that holds mg_solver.c, mg_comm.c, mg_cg.c, mg_gmres.c and the
host-memory stand-ins (tests/mock_mgk_cg.cpp) in place of libmgk.so / libmgpetsc.so.  A process of its own, because the loader caches the
libraries it hands out.  argv: library, output .npz, then one case per argument in the spelling of cg_reference.key."""
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
    import cg_reference as R
    import rhs_cases
    from multigrid_petsc_amd.solver import MgError, Solver
    lib.mock_cg_calls.restype = ctypes.c_int
    lib.mock_cg_calls.argtypes = [ctypes.c_int]
    lib.mock_cg_fail_malloc.argtypes = [ctypes.c_long]
    calls = lambda: np.array([lib.mock_cg_calls(q) for q in range(3)])
    res = {}

    def rhs_of(case, seed=None):
        dim, npts, rhs = case[0], case[1], case[5]
        if seed is not None:
            return rhs_cases.uniform(dim, npts, seed)
        return None if rhs == "manufactured" else rhs_cases.uniform(dim, npts, int(rhs.split(":")[1]))

    def make(case, b, **kw):
        dim, npts, levels, scale, v, rhs, maxiter = case
        s = Solver(dim, npts, levels, v=v, maxiter=maxiter, scale=scale, **kw)
        if b is None:
            s.set_rhs_problem()
        else:
            s.set_rhs(b)
        return s

    for text in sys.argv[3:]:
        case = R.parse(text)
        k = text + ":"
        b = rhs_of(case)
        fresh = make(case, b)
        res[k + "plain_it"], res[k + "plain_rn"], res[k + "plain_u"] = fresh.solve(), fresh.rnorm, fresh.solution()
        fresh.close()
        s = make(case, b)
        lib.mock_cg_calls_reset()
        it = s.solve_cg()
        res[k + "it"], res[k + "rn"], res[k + "x"], res[k + "calls"], res[k + "bnorm"], res[k + "breakdown"] = it, s.rnorm, s.solution(), calls(), s.bnorm, s.cg_breakdown
        # the same call again: the same bits
        assert s.solve_cg() == it and np.array_equal(s.solution(), res[k + "x"]) and np.array_equal(s.rnorm, res[k + "rn"])
        # a second right-hand side on the live handle: what a fresh solver makes of it, bit for bit
        b2 = rhs_of(case, seed=77)
        s.set_rhs(b2)
        it2, rn2, x2 = s.solve_cg(), s.rnorm, s.solution()
        other = make(case, b2)
        assert other.solve_cg() == it2 and np.array_equal(other.rnorm, rn2) and np.array_equal(other.solution(), x2), "second right-hand side"
        other.close()
        res[k + "it_rhs2"] = it2
        # reset + a plain solve afterwards: a fresh solver's history and field, bit for bit (level 0's b is the caller's again)
        if b is None:
            s.set_rhs_problem()
        else:
            s.set_rhs(b)
        assert s.solve_cg() == it and np.array_equal(s.solution(), res[k + "x"])
        s.reset()
        res[k + "after_it"], res[k + "after_rn"], res[k + "after_u"] = s.solve(), s.rnorm, s.solution()
        s.close()
        # without the coarse-level graph and without any fused pass: the bits of the defaults
        if case in (R.CASES[0], R.CASES[5]):
            for kw in (dict(graph=0), dict(fuse=0)):
                q = make(case, b, **kw)
                assert q.solve_cg() == it and np.array_equal(q.rnorm, res[k + "rn"]) and np.array_equal(q.solution(), res[k + "x"]), kw
                q.close()
    # refusals that need another configuration; the handle stays usable (a plain solve runs)
    for dim, kw, msg in ((3, dict(ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev"), (3, dict(precision="mixed"), "not mixed precision"),
                         (2, dict(mesh=1), "use mg_solver_solve_gmres"), (2, dict(mesh=2), "not symmetric")):
        s = Solver(dim, 17, 3, v=(3, 3), maxiter=20, scale=0.8, **kw)
        s.set_rhs_problem()
        try:
            s.solve_cg()
            raise SystemExit(f"{kw} was accepted")
        except MgError as e:
            assert "mg_solver_solve_cg" in str(e) and msg in str(e), str(e)
        assert s.cg_breakdown == 0
        assert s.solve() >= 1
        s.close()
    # the five fields do not fit: the error names the count and the bytes, nothing stays allocated, and the next call succeeds
    s = Solver(2, 33, 4, v=(3, 3), maxiter=20, scale=0.8)
    s.set_rhs_problem()
    lib.mock_cg_fail_malloc(3)
    try:
        s.solve_cg()
        raise SystemExit("the failed allocation went unnoticed")
    except MgError as e:
        assert "needs 5 fine-level fields of" in str(e) and "bytes" in str(e), str(e)
    res["alloc_retry_it"] = s.solve_cg()
    # no step: maxiter 0 and a zero right-hand side
    s.close()
    s = Solver(2, 33, 4, v=(3, 3), maxiter=0, scale=0.8)
    s.set_rhs_problem()
    assert s.solve_cg() == 0 and not s.solution().any() and s.cg_breakdown == 0
    s.close()
    s = Solver(2, 33, 4, v=(3, 3), maxiter=20, scale=0.8)
    s.set_rhs(np.zeros(31 * 31))
    assert s.solve_cg() == 0 and not s.solution().any() and s.bnorm == 0.0
    s.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
