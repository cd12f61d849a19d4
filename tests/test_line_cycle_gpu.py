"""Solver(pc_type="yline", scale=0.8) on the GPU against tests/line_reference.py (the numpy statement of the y-line cycle over the oracle's
assembled rows and transfers).

  cases          npts 65 and 129 on meshes 0 and 1, npts 17 on mesh 2, levels down to 1 x 1; the manufactured right-hand side and a rough one
                 (tests/rhs_cases.uniform; LR.CASES)
  checks         the same cycle count (compared only where the reference's stop decision is clear of rounding: last norm <= 0.8, the one
                 before >= 1.5 rtol ||b||), the history within 1e-12 of rnorm[0], u bit for bit
  invariances    graph=0 gives the bits of the defaults (count, history, u) and reset() + solve() repeats them; fuse=0 gives the same count and
                 the same bits of u.  Its norms come from another reduction (mgk_residual_f64 + mgk_sumsq_f64 instead of the fused
                 mgk_residual_sumsq_*): two orders of summing N <= 16129 non-negative squares differ by at most a few log2(N) eps in the sum
                 (blocked / pairwise partial sums; half of it after the square root), i.e. ~1e-14, so every norm of the history is held to 1e-13
                 of ITSELF -- the bound tests/test_vcycle_gpu.py::test_unfused_final_residual_same_history sets for the same pair of
                 kernels, and far inside the 1e-12 of rnorm[0] that the history is held to against the reference.  fuse=1 keeps that
                 reduction and turns every other fusion off: count, history and u bit for bit, so only the norm reduction is exempt
  the point      npts 513 on mesh 1: the count of the reference (10), below a quarter of the count of pc_type="jacobi" on the same configuration
  refusals       3-D, mixed precision, Chebyshev, nranks > 1 at creation; fmg, solve_fmg and solve_gmres on a line solver"""
import numpy as np
import pytest

import line_reference as LR
from oracle import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _solver(case, **kw):
    import rhs_cases
    from multigrid_petsc_amd.solver import Solver
    npts, levels, mesh, rhs = case
    kw.setdefault("pc_type", "yline")
    s = Solver(2, npts, levels, v=(3, 3), maxiter=kw.pop("maxiter", 100), scale=LR.SCALE, mesh=mesh, **kw)
    if rhs == "manufactured":
        s.set_rhs_problem()
    else:
        s.set_rhs(rhs_cases.uniform(2, npts, int(rhs.split(":")[1])))
    return s


@pytest.mark.parametrize("case", LR.CASES, ids=[LR.case_key(c) for c in LR.CASES])
def test_line_solve_equals_the_reference(orc, case):
    ref = LR.reference(orc, case)
    s = _solver(case)
    it = s.solve()
    rn, u, bn = s.rnorm, s.solution(), s.bnorm
    print(f"{LR.case_key(case)}: {it} cycles (reference {ref['iters']}), max history diff / rnorm[0] = "
          f"{np.abs(rn[:min(len(rn), len(ref['rnorm']))] - ref['rnorm'][:min(len(rn), len(ref['rnorm']))]).max() / ref['rnorm'][0]:.2e}, "
          f"u differs in {int(np.sum(u != ref['u']))} of {u.size}")
    LR.compare(ref, it, rn, u, bn)
    # again on the same solver: the recorded coarse-level graph is replayed from fresh state
    s.reset()
    assert s.solve() == it and np.array_equal(s.rnorm, rn) and np.array_equal(s.solution(), u)
    s.close()
    t = _solver(case, graph=0)
    assert t.solve() == it and np.array_equal(t.rnorm, rn) and np.array_equal(t.solution(), u), "graph=0"
    t.close()
    t = _solver(case, fuse=0)
    itf, rnf, uf = t.solve(), t.rnorm, t.solution()
    t.close()
    print(f"  fuse=0: {itf} cycles, max |rnorm / rnorm_default - 1| = {np.abs(rnf[:len(rn)] / rn[:len(rnf)] - 1).max():.2e}, "
          f"u differs in {int(np.sum(uf != u))} of {u.size}")
    assert itf == it and np.array_equal(uf, u)
    assert np.abs(rnf / rn - 1).max() <= 1e-13
    LR.compare(ref, itf, rnf, uf, bn)
    # bit 0 alone (the fused residual + norm kept, every other fusion off): the whole cycle, history included, bit for bit
    t = _solver(case, fuse=1)
    assert t.solve() == it and np.array_equal(t.rnorm, rn) and np.array_equal(t.solution(), u), "fuse=1"
    t.close()


def test_line_relaxation_is_what_mesh_1_needs(orc):
    """npts 513, -mesh 1: the y-line cycle takes the reference's count, below a quarter of what point Jacobi takes on the same configuration"""
    case = (513, 9, 1, "manufactured")
    ref = LR.reference(orc, case)
    s = _solver(case)
    it = s.solve()
    rn, u, bn = s.rnorm, s.solution(), s.bnorm
    s.close()
    p = _solver(case, pc_type="jacobi", maxiter=400)
    itp = p.solve()
    p.close()
    print(f"513^2 mesh 1: yline {it} cycles (reference {ref['iters']}), jacobi {itp}")
    LR.compare(ref, it, rn, u, bn)
    assert 4 * it < itp, (it, itp)


def test_what_the_line_smoother_is_not_built_for_is_refused():
    from multigrid_petsc_amd.solver import MgError, Solver
    for kw, msg in ((dict(dim=3, npts=17, levels=3), "built for 2-D"),
                    (dict(dim=2, npts=17, levels=3, precision="mixed"), "not mixed precision"),
                    (dict(dim=2, npts=17, levels=3, ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev"),
                    (dict(dim=2, npts=17, levels=3, nranks=2), "one GPU")):
        with pytest.raises(MgError, match=msg):
            Solver(v=(3, 3), maxiter=20, scale=LR.SCALE, pc_type="yline", **kw)
    s = _solver((17, 4, 1, "manufactured"))
    for call in (lambda: s.fmg(1), lambda: s.solve_fmg(1), lambda: s.solve_gmres(30)):
        with pytest.raises(MgError, match="not the y-line smoother"):
            call()
    # the refusals leave the solver usable
    assert s.solve() == 9
    s.close()
