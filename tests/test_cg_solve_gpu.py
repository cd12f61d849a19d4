"""mg_solver_solve_cg on the GPU against tests/cg_reference.py (numpy over the CPU oracle): whole solves on the product's libraries.

Every case of cg_reference.CASES (converged, widths that are not 2^k + 1, capped) through cg_reference.judge -- equal step counts in both
orders of summation, a stop decision clear of rounding, x and the history within max(100 delta, 1e-13) of the nearer order, a converged true
residual -- plus two sizes at which the marching and full-row passes of the cycle, the coarse-level graph and the LDS tail run under CG:
2-D npts 1025 (10 levels) and 3-D npts 129 (6 levels), scale 0.8, V(3,3), rough right-hand sides.  The reference's margins, computed on the
CPU: 129^3 stops after 7 steps at 0.17 / 2.2 rtol ||b||, clear; 1025^2 stops after 6 steps at 0.04 / 1.09 -- the step before is NOT clear
of rounding, so that case is capped at maxiter 5.  The breakdown case, a plain solve afterwards, a repeated call, and the own driver."""
import os
import re
import subprocess

import numpy as np
import pytest

import cg_reference as R
from oracle import Oracle

pytestmark = pytest.mark.gpu
RTOL = 1.0e-7
BIG_CAPPED = (2, 1025, 10, 0.8, (3, 3), "rough:6", 5)
BIG_3D = (3, 129, 6, 0.8, (3, 3), "rough:8", 100)
CASES = R.CASES + [BIG_CAPPED, BIG_3D]
R.CAPPED.append(BIG_CAPPED)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


_REF = {}


def _reference(orc, case):
    if case not in _REF:
        _REF[case] = R.reference(orc, case, RTOL)
    return _REF[case]


def _solver(case, b):
    from multigrid_petsc_amd.solver import Solver
    dim, npts, levels, scale, v, rhs, maxiter = case
    s = Solver(dim, npts, levels, v=v, maxiter=maxiter, scale=scale, rtol=RTOL)
    if rhs == "manufactured":
        s.set_rhs_problem()
    else:
        s.set_rhs(b)
    return s


@pytest.mark.parametrize("case", CASES, ids=[R.key(c) for c in CASES])
def test_solve_cg_equals_the_reference(orc, case):
    b, refs = _reference(orc, case)
    s = _solver(case, b)
    try:
        it = s.solve_cg()
        x, rn = s.solution(), s.rnorm
        dist = min(R.distance(x, rn, r) for r in refs) if it == refs[0]["iters"] else float("nan")
        print(f"\ncg {R.key(case)}: steps {it} (reference {refs[0]['iters']}), delta {R.delta(refs[0], refs[1]):.2e}, GPU distance {dist:.2e}, "
              f"last / (rtol ||b||) {rn[-1] / (RTOL * s.bnorm):.6f}, breakdown {s.cg_breakdown}, seconds {s.solve_seconds:.6f}")
        R.judge(orc, case, b, refs, it, rn, x, s.bnorm, RTOL)
        assert s.cg_breakdown == 0 and s.solve_seconds > 0.0
        # a second call reproduces the first, bit for bit
        assert s.solve_cg() == it and np.array_equal(s.solution(), x) and np.array_equal(s.rnorm, rn)
    finally:
        s.close()


@pytest.mark.parametrize("case", [R.CONVERGED[1], R.CONVERGED[5], R.OFF_WIDTH[2]], ids=[R.key(c) for c in (R.CONVERGED[1], R.CONVERGED[5], R.OFF_WIDTH[2])])
def test_plain_solve_after_cg_equals_a_fresh_solver(orc, case):
    b, refs = _reference(orc, case)
    fresh, s = _solver(case, b), _solver(case, b)
    try:
        itf = fresh.solve()
        xf, rnf = fresh.solution(), fresh.rnorm
        s.solve_cg()
        s.reset()
        assert s.solve() == itf
        assert np.array_equal(s.rnorm, rnf) and np.array_equal(s.solution(), xf)
    finally:
        fresh.close(); s.close()


def test_cg_converges_at_richardson_scale_one_where_the_cycle_alone_does_not(orc):
    for case in (R.CONVERGED[1], R.CONVERGED[6]):
        b, refs = _reference(orc, case)
        s = _solver(case, b)
        try:
            assert s.solve() == 100 and s.rnorm[-1] > RTOL * s.bnorm        # undamped Jacobi is not a smoother
            s.reset()
            assert s.solve_cg() == refs[0]["iters"] and s.rnorm[-1] <= RTOL * s.bnorm
        finally:
            s.close()


def test_breakdown_refusals_and_zero_right_hand_side(orc):
    from multigrid_petsc_amd.solver import MgError, Solver
    b, refs = _reference(orc, R.BREAKDOWN)
    assert [r["breakdown"] for r in refs] == [1, 1]
    s = _solver(R.BREAKDOWN, b)
    try:
        assert s.solve_cg() == 0 and s.cg_breakdown == 1 and not s.solution().any() and len(s.rnorm) == 1
        s.set_rhs(np.zeros(s.local_unknowns))
        assert s.solve_cg() == 0 and s.cg_breakdown == 0 and not s.solution().any()
    finally:
        s.close()
    for dim, kw, msg in ((2, dict(ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev"), (3, dict(precision="mixed"), "not mixed precision"),
                         (2, dict(pc_type="rbgs"), "built for point Jacobi"), (2, dict(pc_type="yline"), "built for point Jacobi"),
                         (2, dict(mesh=1), "use mg_solver_solve_gmres")):
        q = Solver(dim, 33, 4, v=(3, 3), maxiter=50, scale=0.8, **kw)
        try:
            q.set_rhs_problem()
            with pytest.raises(MgError, match=msg):
                q.solve_cg()
            assert q.solve() >= 1                                   # the handle is as usable as before
        finally:
            q.close()


def test_own_driver_with_mg_krylov_cg(orc, tmp_path):
    """mgpoisson -mg_krylov cg at PETSc's default scale 1: the lines of a plain solve, the reference's step count, a converged relative
    residual and the history in rData.dat; without the option the plain iteration runs into its cap"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "multigrid_petsc_amd", "mgpoisson")
    case = R.CONVERGED[1]
    b, refs = _reference(orc, case)
    base = ["-dim", "2", "-npts", "65", "-levels", "5", "-ksp_richardson_scale", "1.0", "-iter", "100", "-v", "3,3", "-write_fields", "0"]
    out = {}
    for tag, extra in (("cg", ["-mg_krylov", "cg"]), ("plain", ["-mg_krylov", "none"])):
        p = subprocess.run([exe] + base + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-2000:]
        out[tag] = (int(re.search(r"Number of iterations:\s+(\d+)", p.stdout).group(1)), float(re.search(r"Relative residual = (\S+)", p.stdout).group(1)),
                    np.array(open(tmp_path / "rData.dat").read().split(), dtype=float))
        assert "Solver walltime" in p.stdout and "error[2]" in p.stdout
    it, rel, hist = out["cg"]
    assert it == refs[0]["iters"] and rel <= RTOL and len(hist) == it + 1 and hist[0] == 1.0
    assert np.abs(hist - refs[0]["rnorm"] / refs[0]["rnorm"][0]).max() <= 1e-10
    assert out["plain"][0] == 100 and out["plain"][1] > RTOL
