"""mg_solver_solve_cg_mixed on the GPU against tests/cg_mixed_reference.py (numpy over the CPU oracle's mixed cycle): whole solves on the product's
libraries, precision="mixed".

Every case of cg_mixed_reference.CASES (converged, a width that is not 2^k + 1, capped at scale 1) through cg_reference.judge -- equal step counts
in both orders of summation, a stop decision clear of rounding, x and the history within max(100 delta, 1e-13) of the nearer order, a converged
true residual -- plus 129^3 with 6 levels.  A plain mixed solve afterwards, a repeated call, the scale-1 case that the plain mixed iteration does not converge on, the
breakdown case, and the own driver."""
import os
import re
import subprocess

import numpy as np
import pytest

import cg_mixed_reference as R
from oracle import Oracle

pytestmark = pytest.mark.gpu
RTOL = 1.0e-7
DRIVER_CASE = (3, 17, 3, 0.8, (3, 3), "manufactured", 100)
# one size at which the marching passes of the fp32 cycle, the coarse-level graph and the LDS tail run under CG.  The reference on the CPU: 7 steps,
# 0.17 / 2.23 rtol ||b||, clear of rounding (delta 1.3e-12)
BIG_3D = (3, 129, 6, 0.8, (3, 3), "rough:8", 100)
CASES = R.CASES + [BIG_3D]


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
    s = Solver(dim, npts, levels, v=v, maxiter=maxiter, scale=scale, rtol=RTOL, precision="mixed")
    s.set_rhs(b)
    return s


@pytest.mark.parametrize("case", CASES, ids=[R.key(c) for c in CASES])
def test_solve_cg_mixed_equals_the_reference(orc, case):
    b, refs = _reference(orc, case)
    s = _solver(case, b)
    try:
        it = s.solve_cg_mixed()
        x, rn = s.solution(), s.rnorm
        dist = min(R.distance(x, rn, r) for r in refs) if it == refs[0]["iters"] else float("nan")
        print(f"\ncg_mixed {R.key(case)}: steps {it} (reference {refs[0]['iters']}), delta {R.delta(refs[0], refs[1]):.2e}, GPU distance {dist:.2e}, "
              f"last / (rtol ||b||) {rn[-1] / (RTOL * s.bnorm):.6f}, breakdown {s.cg_breakdown}, seconds {s.solve_seconds:.6f}")
        R.judge(orc, case, b, refs, it, rn, x, s.bnorm, RTOL)
        assert s.cg_breakdown == 0 and s.solve_seconds > 0.0
        # a second call reproduces the first, bit for bit
        assert s.solve_cg_mixed() == it and np.array_equal(s.solution(), x) and np.array_equal(s.rnorm, rn)
    finally:
        s.close()


@pytest.mark.parametrize("case", [R.CONVERGED[0], R.OFF_WIDTH[0]], ids=[R.key(c) for c in (R.CONVERGED[0], R.OFF_WIDTH[0])])
def test_plain_mixed_solve_after_cg_equals_a_fresh_solver(orc, case):
    b, refs = _reference(orc, case)
    fresh, s = _solver(case, b), _solver(case, b)
    try:
        itf = fresh.solve()
        xf, rnf = fresh.solution(), fresh.rnorm
        s.solve_cg_mixed()
        s.reset()
        assert s.solve() == itf
        assert np.array_equal(s.rnorm, rnf) and np.array_equal(s.solution(), xf)
    finally:
        fresh.close(); s.close()


def test_cg_converges_at_scale_one_where_the_plain_mixed_iteration_does_not(orc):
    case = R.SCALE_ONE
    b, refs = _reference(orc, case)
    assert refs[0]["iters"] == refs[1]["iters"] == 30
    s = _solver(case, b)
    try:
        assert s.solve() == 100 and s.rnorm[-1] > RTOL * s.bnorm            # undamped Jacobi is not a smoother, in fp32 as in fp64
        s.reset()
        assert s.solve_cg_mixed() == 30 and s.cg_breakdown == 0 and s.rnorm[-1] <= RTOL * s.bnorm
        op = R.MixedOperators(orc, case)
        r = b - op.A(s.solution())
        op.close()
        assert np.sqrt(np.dot(r, r)) <= RTOL * s.bnorm * (1.0 + 1e-3)
    finally:
        s.close()


def test_breakdown_refusals_and_zero_right_hand_side(orc):
    from multigrid_petsc_amd.solver import MgError, Solver
    b, refs = _reference(orc, R.BREAKDOWN)
    assert refs[0]["breakdown"] == refs[1]["breakdown"] >= 1 and refs[0]["iters"] == refs[1]["iters"]
    s = _solver(R.BREAKDOWN, b)
    try:
        it = s.solve_cg_mixed()
        assert it == refs[0]["iters"] and s.cg_breakdown == refs[0]["breakdown"] and len(s.rnorm) == it + 1
        assert min(R.distance(s.solution(), s.rnorm, r) for r in refs) <= max(100.0 * R.delta(refs[0], refs[1]), 1e-13)
        s.set_rhs(np.zeros(s.local_unknowns))
        assert s.solve_cg_mixed() == 0 and s.cg_breakdown == 0 and not s.solution().any()
        with pytest.raises(MgError, match="not mixed precision"):
            s.solve_cg()
    finally:
        s.close()
    q = Solver(3, 33, 4, v=(3, 3), maxiter=50, scale=0.8)
    try:
        q.set_rhs_problem()
        with pytest.raises(MgError, match="built for a mixed-precision solver"):
            q.solve_cg_mixed()
        assert q.solve() >= 1                                       # the handle is as usable as before
    finally:
        q.close()


def test_own_driver_with_mg_krylov_cg_and_precision_mixed(orc, tmp_path):
    """mgpoisson -precision mixed -mg_krylov cg: the lines of a plain solve, the reference's step count for the manufactured right-hand side (its
    stop decision is clear of rounding: asserted), a converged relative residual and the history in rData.dat"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "multigrid_petsc_amd", "mgpoisson")
    op = R.MixedOperators(orc, DRIVER_CASE)
    ref = R.cg(op, op.rhs(), rtol=RTOL, maxiter=100)
    op.close()
    last, before = R.margins(ref, RTOL)
    assert ref["breakdown"] == 0 and last <= 0.8 and before >= 1.5
    args = ["-dim", "3", "-npts", "17", "-levels", "3", "-ksp_richardson_scale", "0.8", "-iter", "100", "-v", "3,3", "-write_fields", "0", "-precision", "mixed",
            "-mg_krylov", "cg"]
    p = subprocess.run([exe] + args, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:]
    it = int(re.search(r"Number of iterations:\s+(\d+)", p.stdout).group(1))
    rel = float(re.search(r"Relative residual = (\S+)", p.stdout).group(1))
    hist = np.array(open(tmp_path / "rData.dat").read().split(), dtype=float)
    assert "Solver walltime" in p.stdout and "error[2]" in p.stdout
    assert it == ref["iters"] and rel <= RTOL and len(hist) == it + 1 and hist[0] == 1.0
    assert np.abs(hist - ref["rnorm"] / ref["rnorm"][0]).max() <= 1e-10
