"""Solver(pc_type="altline" | "xline", scale=0.8) on the GPU against tests/xline_reference.py (the numpy statement of the x-line sweep and of
the alternating cycle over the oracle's assembled rows and transfers).

  cases          the cases of the CPU tier up to npts 129 (XR.CASES: meshes 0 / 1 / 2, levels down to 1 x 1, the manufactured right-hand side
                 and rough ones), every one with a stop decision clear of rounding
  checks         the same cycle count (the pinned one), the history within 1e-12 of rnorm[0], u bit for bit
  invariances    graph=0 gives the bits of the defaults (count, history, u) and reset() + solve() repeats them
  neighbours     a yline solve made before and after an altline solve in the same process: bit-identical
  other counts   v = (2, 1) and (1, 2): the reference's count and solution (every smoothing starts with a y sweep, the coarsest level's too)
  refusals       3-D, mixed precision, Chebyshev, nranks > 1 at creation; fmg, solve_fmg and solve_gmres on such a solver"""
import numpy as np
import pytest

import line_reference as LR
import xline_reference as XR
from oracle import Oracle

pytestmark = pytest.mark.gpu
CASES = [c for c in XR.CASES if c[1] <= 129]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _solver(case, v=(3, 3), **kw):
    import rhs_cases
    from multigrid_petsc_amd.solver import Solver
    pc, npts, levels, mesh, rhs = case[:5]
    s = Solver(2, npts, levels, v=v, maxiter=100, scale=XR.SCALE, mesh=mesh, pc_type=pc, **kw)
    if rhs == "manufactured":
        s.set_rhs_problem()
    else:
        s.set_rhs(rhs_cases.uniform(2, npts, int(rhs.split(":")[1])))
    return s


@pytest.mark.parametrize("case", CASES, ids=[XR.xcase_key(c) for c in CASES])
def test_solve_equals_the_reference(orc, case):
    ref = XR.reference(orc, case)
    assert ref["iters"] == case[5]
    s = _solver(case)
    it = s.solve()
    rn, u, bn = s.rnorm, s.solution(), s.bnorm
    m = min(len(rn), len(ref["rnorm"]))
    print(f"{XR.xcase_key(case)}: {it} cycles (reference {ref['iters']}), max history diff / rnorm[0] = "
          f"{np.abs(rn[:m] - ref['rnorm'][:m]).max() / ref['rnorm'][0]:.2e}, u differs in {int(np.sum(u != ref['u']))} of {u.size}")
    XR.compare(ref, it, rn, u, bn)
    # again on the same solver: the recorded coarse-level graph is replayed from fresh state
    s.reset()
    assert s.solve() == it and np.array_equal(s.rnorm, rn) and np.array_equal(s.solution(), u)
    s.close()
    t = _solver(case, graph=0)
    assert t.solve() == it and np.array_equal(t.rnorm, rn) and np.array_equal(t.solution(), u), "graph=0"
    t.close()


@pytest.mark.parametrize("v", [(2, 1), (1, 2)])
def test_other_sweep_counts(orc, v):
    case = ("altline", 33, 5, 2, "manufactured")
    h = XR.Hierarchy(orc, 33, 5, 2, "altline")
    ref = XR.solve(h, h.rhs(), XR.SCALE, v=v, rtol=XR.RTOL, maxiter=100)
    for graph in (1, 0):
        s = _solver(case, v=v, graph=graph)
        it = s.solve()
        print(f"v = {v}, graph = {graph}: {it} cycles (reference {ref['iters']})")
        assert it == ref["iters"] and np.array_equal(s.solution(), ref["u"])
        assert np.abs(s.rnorm - ref["rnorm"]).max() <= 1e-12 * ref["rnorm"][0]
        s.close()


def test_a_yline_solve_before_and_after_an_altline_solve(orc):
    ycase = ("yline", 65, 6, 1, "manufactured")
    ref = LR.reference(orc, (65, 6, 1, "manufactured"))
    y = _solver(ycase)
    it = y.solve()
    rn, u = y.rnorm, y.solution()
    LR.compare(ref, it, rn, u, y.bnorm)
    a = _solver(("altline", 65, 6, 2, "manufactured"))
    assert a.solve() == 8
    y.reset()
    assert y.solve() == it and np.array_equal(y.rnorm, rn) and np.array_equal(y.solution(), u)
    y.close()
    y2 = _solver(ycase)
    assert y2.solve() == it and np.array_equal(y2.rnorm, rn) and np.array_equal(y2.solution(), u)
    y2.close()
    a.close()


def test_what_the_line_smoothers_are_not_built_for_is_refused():
    from multigrid_petsc_amd.solver import MgError, Solver
    for pc, name in (("xline", "x-line"), ("altline", "alternating line")):
        for kw, msg in ((dict(dim=3, npts=17, levels=3), "built for 2-D"),
                        (dict(dim=2, npts=17, levels=3, precision="mixed"), "not mixed precision"),
                        (dict(dim=2, npts=17, levels=3, ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev"),
                        (dict(dim=2, npts=17, levels=3, nranks=2), "one GPU")):
            with pytest.raises(MgError) as e:
                Solver(v=(3, 3), maxiter=20, scale=XR.SCALE, pc_type=pc, **kw)
            assert msg in str(e.value) and f"the {name} smoother" in str(e.value), str(e.value)
        s = _solver((pc, 17, 4, 0, "manufactured"))
        for call in (lambda: s.fmg(1), lambda: s.solve_fmg(1), lambda: s.solve_gmres(30)):
            with pytest.raises(MgError, match="not the x-line or alternating line smoothers"):
                call()
        # the refusals leave the solver usable
        assert s.solve() == 7
        s.close()
    with pytest.raises(KeyError):
        Solver(2, 17, 4, pc_type="zebra")
