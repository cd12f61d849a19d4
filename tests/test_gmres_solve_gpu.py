"""mg_solver_solve_gmres on the GPU against tests/gmres_reference.py (numpy over the CPU oracle): whole solves.

Cases (dim, npts, levels, mesh, scale, restart, right-hand side, maxiter): uniform and both stretched meshes in 2-D, 3-D, a rough right-hand
side across two restarts (restart 5), PETSc's default Richardson scale 1, and 1025^2 on mesh 1 -- large enough for the three-sweep passes,
the coarse-level graph and the LDS tail -- capped at 6 steps because its reference costs about a second per application of M.

  count       equal to the reference's.  First, for BOTH dot variants of the reference: the last estimate is <= 0.8 rtol ||b|| and the one
              before >= 1.5 rtol ||b|| (the capped case: every estimate >= 1.5 rtol ||b||, so the cap decides), else rounding could decide.
  x, history  bit equality is not available (the scalars come from sums whose order differs).  delta = the larger of
              max|x_a - x_b| / max|x_b| and max_k |rnorm_a[k] - rnorm_b[k]| / rnorm[0] between the reference's two dot variants (np.dot, long
              double) is what one change of summation order does; the GPU must lie within 100 delta (floor 1e-13) of either variant: the
              factor because one pair of orders is a single sample of that spread.  Histories relative to rnorm[0], not entry by entry.
  converged   ||b - A x|| of the GPU's x, evaluated by the oracle, is <= rtol ||b|| (1 + 100 eps), eps = the reference's own relative gap
              between its last estimate and its true residual (the capped case: <= the GPU's last estimate times that factor).
  accelerates fewer applications of M than solve() takes cycles (mesh 1 and mesh 2); at scale 1 within 10 steps where solve() has not
              converged within 100.
  state       reset + solve reproduces a fresh solver bit for bit (level 0's b is the caller's again); a second solve_gmres reproduces the
              first; another restart length reallocates and, being longer than the solve, gives the same bits; refusals."""
import numpy as np
import pytest

import gmres_reference as G
import rhs_cases
from oracle import Oracle

pytestmark = pytest.mark.gpu
RTOL = 1.0e-7
# (dim, npts, levels, mesh, scale, restart, rhs, maxiter); rough = rhs_cases.uniform with the seed that follows the name
CASES = [
    (2, 65, 5, 0, 0.8, 30, "manufactured", 100),
    (2, 65, 5, 1, 0.8, 30, "manufactured", 100),
    (2, 65, 5, 1, 0.8, 5, "rough:12", 100),
    (2, 65, 5, 2, 0.8, 30, "manufactured", 100),
    (3, 33, 4, 0, 0.8, 30, "rough:3", 100),
    (3, 33, 4, 0, 1.0, 4, "manufactured", 100),
    (2, 1025, 9, 1, 0.8, 30, "manufactured", 6),
]
IDS = ["uniform", "mesh1", "mesh1-rough-restart5", "mesh2", "3d-rough", "3d-scale1-restart4", "1025-mesh1-capped"]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


_REF = {}


def _rhs(op, rhs, dim, npts):
    if rhs == "manufactured":
        return op.rhs()
    return rhs_cases.uniform(dim, npts, int(rhs.split(":")[1]))


def _reference(orc, case):
    """both dot variants of the reference, computed once per case and shared"""
    if case not in _REF:
        dim, npts, levels, mesh, scale, restart, rhs, maxiter = case
        op = G.Operators(orc, dim, npts, levels, mesh, scale)
        b = _rhs(op, rhs, dim, npts)
        refs = [G.gmres(op, b, restart, rtol=RTOL, maxiter=maxiter, dot=d) for d in ("np", "ld")]
        op.close()
        _REF[case] = (b, refs)
    return _REF[case]


def _solver(case, b):
    from multigrid_petsc_amd.solver import Solver
    dim, npts, levels, mesh, scale, restart, rhs, maxiter = case
    s = Solver(dim, npts, levels, v=(3, 3), maxiter=maxiter, scale=scale, mesh=mesh, rtol=RTOL)
    if rhs == "manufactured":
        s.set_rhs_problem()
    else:
        s.set_rhs(b)
    return s


def _true_residual(orc, case, b, x):
    dim, npts, levels, mesh, scale = case[:5]
    op = G.Operators(orc, dim, npts, levels, mesh, scale)
    r = b - op.A(x)
    op.close()
    return float(np.sqrt(np.dot(r, r)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_solve_gmres_equals_the_reference(orc, case):
    dim, npts, levels, mesh, scale, restart, rhs, maxiter = case
    b, refs = _reference(orc, case)
    capped = maxiter < 100
    for r in refs:
        q = r["rnorm"] / (RTOL * r["bnorm"])
        if capped:
            assert r["iters"] == maxiter and q.min() >= 1.5, q
        else:
            last, before = G.margins(r, RTOL)
            assert last <= 0.8 and before >= 1.5, (last, before)
    assert refs[0]["iters"] == refs[1]["iters"]
    s = _solver(case, b)
    try:
        it = s.solve_gmres(restart)
        x, rn = s.solution(), s.rnorm
        assert it == refs[0]["iters"], (it, refs[0]["iters"])
        assert len(rn) == it + 1
        assert abs(s.bnorm - refs[0]["bnorm"]) <= 1e-13 * refs[0]["bnorm"] and rn[0] == s.bnorm
        assert s.solve_seconds > 0.0
        delta = G.delta(refs[0], refs[1])
        bound = max(100.0 * delta, 1e-13)
        dist = min(G.distance(x, rn, r) for r in refs)
        true = _true_residual(orc, case, b, x)
        eps = max(abs(r["rnorm"][-1] - r["true"]) / r["true"] for r in refs)
        print(f"\ngmres {IDS[CASES.index(case)]}: steps {it}, applications of M {refs[0]['napply']}, delta {delta:.2e}, bound {bound:.2e}, "
              f"GPU distance {dist:.2e}, eps {eps:.2e}, true residual / (rtol ||b||) {true / (RTOL * s.bnorm):.6f}, "
              f"last estimate / (rtol ||b||) {rn[-1] / (RTOL * s.bnorm):.6f}")
        assert dist <= bound, (dist, bound)
        if capped:
            assert true <= rn[-1] * (1.0 + 100.0 * eps), (true, rn[-1], eps)
        else:
            assert true <= RTOL * s.bnorm * (1.0 + 100.0 * eps), (true, RTOL * s.bnorm, eps)
        # a second call reproduces the first; a longer restart than the solve reallocates and changes nothing
        assert s.solve_gmres(restart) == it
        assert np.array_equal(s.solution(), x) and np.array_equal(s.rnorm, rn)
        if it < restart < 32:
            assert s.solve_gmres(restart + 1) == it
            assert np.array_equal(s.solution(), x) and np.array_equal(s.rnorm, rn)
        else:
            assert s.solve_gmres(restart + 2) >= 1                  # another basis length: allocated anew, runs
    finally:
        s.close()


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[3], CASES[4]], ids=[IDS[1], IDS[2], IDS[3], IDS[4]])
def test_plain_solve_after_gmres_equals_a_fresh_solver(orc, case):
    b, refs = _reference(orc, case)
    fresh = _solver(case, b)
    s = _solver(case, b)
    try:
        itf = fresh.solve()
        xf, rnf = fresh.solution(), fresh.rnorm
        s.solve_gmres(case[5])
        s.reset()
        assert s.solve() == itf
        assert np.array_equal(s.rnorm, rnf) and np.array_equal(s.solution(), xf)
    finally:
        fresh.close(); s.close()


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=[IDS[1], IDS[3]])
def test_gmres_takes_fewer_applications_of_the_cycle(orc, case):
    b, refs = _reference(orc, case)
    restart = case[5]
    s = _solver(case, b)
    try:
        cycles = s.solve()
        assert s.rnorm[-1] <= RTOL * s.bnorm
        s.reset()
        steps = s.solve_gmres(restart)
        applications = steps + -(-steps // restart)                 # one per step and one per correction
        assert applications == refs[0]["napply"]
        print(f"\ngmres {IDS[CASES.index(case)]}: {applications} applications of M against {cycles} V-cycles")
        assert applications < cycles, (applications, cycles)
    finally:
        s.close()


def test_gmres_converges_at_richardson_scale_one_where_the_cycle_alone_does_not(orc):
    case = CASES[5]
    b, refs = _reference(orc, case)
    s = _solver(case, b)
    try:
        assert s.solve() == 100 and s.rnorm[-1] > RTOL * s.bnorm        # undamped Jacobi is not a smoother
        s.reset()
        steps = s.solve_gmres(case[5])
        assert steps <= 10 and s.rnorm[-1] <= RTOL * s.bnorm
    finally:
        s.close()


def test_refusals_and_zero_right_hand_side():
    from multigrid_petsc_amd.solver import MgError, Solver
    s = Solver(2, 33, 4, v=(3, 3), maxiter=50, scale=0.8)
    try:
        s.set_rhs_problem()
        for m in (0, -1, 33, 1000):
            with pytest.raises(MgError, match="restart must be within"):
                s.solve_gmres(m)
        assert s.solve_gmres(32) >= 1 and s.solve_gmres(1) >= 1
        s.set_rhs(np.zeros(s.local_unknowns))
        assert s.solve_gmres(30) == 0 and not s.solution().any()
    finally:
        s.close()
    c = Solver(2, 33, 4, v=(3, 3), maxiter=50, ksp_type="chebyshev", eigenvalues=(0.2, 2.0))
    try:
        c.set_rhs_problem()
        with pytest.raises(MgError, match="not Chebyshev"):
            c.solve_gmres(30)
    finally:
        c.close()
    m = Solver(3, 33, 4, v=(3, 3), maxiter=50, scale=0.8, precision="mixed")
    try:
        m.set_rhs_problem()
        with pytest.raises(MgError, match="not mixed precision"):
            m.solve_gmres(30)
    finally:
        m.close()


def test_own_driver_with_mg_accel_gmres(orc, tmp_path):
    """mgpoisson -mg_accel gmres on mesh 1: the lines of a plain solve, the reference's step count, a converged relative residual, and
    the estimates in rData.dat; without the option the plain iteration's count"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "multigrid_petsc_amd", "mgpoisson")
    case = CASES[1]
    b, refs = _reference(orc, case)
    base = ["-dim", "2", "-npts", "65", "-levels", "5", "-mesh", "1", "-ksp_richardson_scale", "0.8", "-iter", "100", "-v", "3,3", "-write_fields", "0"]
    out = {}
    for tag, extra in (("gmres", ["-mg_accel", "gmres", "-mg_gmres_restart", "30"]), ("plain", [])):
        p = subprocess.run([exe] + base + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-2000:]
        out[tag] = (int(re.search(r"Number of iterations:\s+(\d+)", p.stdout).group(1)), float(re.search(r"Relative residual = (\S+)", p.stdout).group(1)),
                    np.array(open(tmp_path / "rData.dat").read().split(), dtype=float))
        assert "Solver walltime" in p.stdout and "error[2]" in p.stdout
    it, rel, hist = out["gmres"]
    assert it == refs[0]["iters"] and rel <= RTOL and len(hist) == it + 1 and hist[0] == 1.0
    assert np.abs(hist - refs[0]["rnorm"] / refs[0]["rnorm"][0]).max() <= 1e-10
    assert out["plain"][0] > it + 1
