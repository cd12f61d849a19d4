"""Conjugate gradients with the V-cycle as preconditioner in numpy over the CPU oracle: the definition that mg_solver_solve_cg (csrc/mg_cg.c) is
held to.  Test infrastructure only.

  M r   one V(v0,v1) cycle from the zero guess (gmres_reference.Operators.M: Oracle.vcycle(fixed_cycles=1, b=r)), uniform mesh
  A x   Oracle.apply with the level-0 stencil, the canonical order

  x = 0, r = b, z = M r, p = z, rho = r . z
  step k: q = A p; sigma = p . q; alpha = rho / sigma; breakdown unless alpha is finite and > 0
          x = x + alpha p; r = r - alpha q; rnorm[k] = sqrt(r . r)
          stop: rnorm[k] <= rtol ||b||, k = maxiter, or the divergence guard (1e8 ||b|| <= rnorm[k])
          z = M r; rho' = r . z; beta = rho' / rho; breakdown unless beta is finite and >= 0; p = z + beta p; rho = rho'

Every product and every sum of the field updates is rounded separately (numpy does that).  The sums (dots, norms) have no fixed order on the
GPU, so two variants are selectable: dot="np" (np.dot: blocked, pairwise) and dot="ld" (a long-double sum).  The distance between the two is
the measure of what rounding alone does to a solve.  The level operator is negative definite: rho and sigma are negative, alpha positive."""
import math

import numpy as np

import gmres_reference as G
from gmres_reference import Operators, delta, distance, margins  # noqa: F401  (the shared helpers, re-exported)

# (dim, npts, levels, scale, (v0, v1), rhs, maxiter): rhs "manufactured" or "rough:<seed>" (tests/rhs_cases.uniform)
CONVERGED = [
    (2, 65, 5, 0.8, (3, 3), "manufactured", 100),
    (2, 65, 5, 1.0, (3, 3), "manufactured", 100),
    (2, 65, 5, 1.0, (1, 1), "manufactured", 100),
    (2, 129, 6, 0.8, (3, 3), "rough:5", 100),
    (2, 257, 7, 0.8, (2, 1), "rough:9", 100),
    (3, 33, 4, 0.8, (3, 3), "rough:3", 100),
    (3, 33, 4, 1.0, (1, 1), "manufactured", 100),
    (3, 65, 5, 0.8, (3, 3), "rough:7", 100),
]
# widths that are not 2^k + 1 (generic kernel forms, odd tile remainders).  mg_solver_create takes npts - 1 = m 2^(levels-1) with an odd number of
# unknowns on every level only, so the off-width hierarchies are those of tests/offwidth_cases.py, npts - 1 = 3 * 2^k: level widths 95 / 47 / 23,
# 23 / 11 and 23^3 / 11^3 (reference: 24, 13 and 15 steps, margins 0.71 / 2.8, 0.73 / 6.3, 0.56 / 2.6)
OFF_WIDTH = [
    (2, 97, 3, 0.8, (3, 3), "rough:2", 100),
    (2, 25, 2, 0.8, (3, 3), "rough:1", 100),
    (3, 25, 2, 0.8, (3, 3), "rough:2", 100),
]
CAPPED = [              # maxiter below the converged count: many steps at scale 1, no stop decision to be sensitive to
    (2, 65, 5, 1.0, (3, 3), "rough:12", 10),
    (3, 25, 2, 1.0, (3, 3), "rough:4", 6),           # (23 steps to the tolerance)
]
BREAKDOWN = (2, 33, 4, 1.5, (3, 3), "rough:1", 100)      # an over-relaxed smoother: M is indefinite, alpha <= 0 in step 1
CASES = CONVERGED + OFF_WIDTH + CAPPED


def key(case):
    dim, npts, levels, scale, v, rhs, maxiter = case
    return f"{dim},{npts},{levels},{scale!r},{v[0]},{v[1]},{rhs},{maxiter}"


def parse(text):
    f = text.split(",")
    return (int(f[0]), int(f[1]), int(f[2]), float(f[3]), (int(f[4]), int(f[5])), f[6], int(f[7]))


def capped(case):
    return case in CAPPED


def rhs_of(op, case):
    import rhs_cases
    dim, npts, rhs = case[0], case[1], case[5]
    return op.rhs() if rhs == "manufactured" else rhs_cases.uniform(dim, npts, int(rhs.split(":")[1]))


def operators(orc, case):
    dim, npts, levels, scale, v, rhs, maxiter = case
    return Operators(orc, dim, npts, levels, 0, scale, v=v)


def cg(op, b, rtol=1.0e-7, maxiter=100000, dot="np"):
    """returns {"iters", "rnorm" (rnorm[0] = ||b||, rnorm[k] = ||r|| of the recurrence after step k), "x", "bnorm", "napply" (applications of
    M), "breakdown" (the step, 1-based; 0: none), "true" (||b - A x||)}"""
    dt = G._dot(dot)
    b = np.ascontiguousarray(b, dtype=np.float64)
    bnorm = math.sqrt(dt(b, b))
    tol = rtol * bnorm
    x = np.zeros_like(b)
    rn = [bnorm]
    napply0, it, breakdown = op.napply, 0, 0
    if bnorm == 0.0 or maxiter < 1:
        return {"iters": 0, "rnorm": np.array(rn), "x": x, "bnorm": bnorm, "napply": 0, "breakdown": 0, "true": bnorm}
    r = b.copy()
    z = op.M(r)
    p = z
    rho = dt(r, z)
    k = 0
    while True:
        k += 1
        q = op.A(p)
        sigma = dt(p, q)
        with np.errstate(all="ignore"):
            alpha = float(np.float64(rho) / np.float64(sigma))
        if not (math.isfinite(alpha) and alpha > 0.0):
            breakdown = k
            break
        x = x + alpha * p
        r = r - alpha * q
        res = math.sqrt(dt(r, r))
        it = k
        rn.append(res)
        if not (it < maxiter and 100000000 * bnorm > res and res > tol):
            break
        z = op.M(r)
        rho1 = dt(r, z)
        with np.errstate(all="ignore"):
            beta = float(np.float64(rho1) / np.float64(rho))
        if not (math.isfinite(beta) and beta >= 0.0):
            breakdown = k
            break
        p = z + beta * p
        rho = rho1
    rt = b - op.A(x)
    return {"iters": it, "rnorm": np.array(rn), "x": x, "bnorm": bnorm, "napply": op.napply - napply0, "breakdown": breakdown,
            "true": math.sqrt(float(np.dot(rt, rt)))}


def reference(orc, case, rtol=1.0e-7):
    """(b, [the reference in the two orders of summation])"""
    op = operators(orc, case)
    b = rhs_of(op, case)
    refs = [cg(op, b, rtol=rtol, maxiter=case[6], dot=d) for d in ("np", "ld")]
    op.close()
    return b, refs


def judge(orc, case, b, refs, it, rn, x, bnorm, rtol=1.0e-7):
    """The bars a solve_cg result (it, rn, x, bnorm) is held to on `case` and the right-hand side b, against refs = the reference's two orders
    of summation: the same count in both; for a converged case a stop decision clear of rounding (last entry <= 0.8, the one before >= 1.5, in
    units of rtol ||b||) and a converged TRUE residual; for a capped case the count is maxiter; the history's length and first entry; x and the
    history within max(100 delta, 1e-13) of the nearer variant (delta = the distance between the two)."""
    dim, npts, levels, scale, v, rhs, maxiter = case
    assert refs[0]["breakdown"] == refs[1]["breakdown"] == 0
    if capped(case):
        assert refs[0]["iters"] == refs[1]["iters"] == maxiter
    else:
        for r in refs:
            last, before = margins(r, rtol)
            assert last <= 0.8 and before >= 1.5, (last, before)
    assert it == refs[0]["iters"] == refs[1]["iters"], (it, refs[0]["iters"], refs[1]["iters"])
    assert len(rn) == it + 1 and rn[0] == bnorm and abs(bnorm - refs[0]["bnorm"]) <= 1e-13 * bnorm
    bound = max(100.0 * delta(refs[0], refs[1]), 1e-13)
    dist = min(distance(x, rn, r) for r in refs)
    assert dist <= bound, (dist, bound)
    if not capped(case):
        op = operators(orc, case)
        r = b - op.A(np.asarray(x))
        op.close()
        eps = max(abs(q["rnorm"][-1] - q["true"]) / q["true"] for q in refs)
        assert np.sqrt(np.dot(r, r)) <= rtol * bnorm * (1.0 + 100.0 * eps)
