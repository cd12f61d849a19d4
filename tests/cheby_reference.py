"""The restarted Chebyshev recurrence of the smoother (KSPCHEBYSHEV with Jacobi, PETSc's classic three-term form) restated over the
oracle's primitives, for the tests of the fused Chebyshev passes.  The factors are the expressions of oracle/mgo.c (smooth) in the same
order; Python floats are IEEE doubles, so they carry the same bits."""
import numpy as np

from row_tables import _rt_apply, _rt_jacobi

EIGS = [(0.2, 2.0), (0.5, 2.0), (0.05, 1.7)]      # the last two give omega > 1, i.e. 1 - omega < 0, in the steps 2 and 3


def cheb_steps(emin, emax, nsteps):
    """(s, [(1 - omega, omega, omega * Gamma * s) for the steps 2 .. nsteps])"""
    scale = 2.0 / (emax + emin)
    alpha = 1.0 - scale * emin
    Gamma = 1.0
    mu = 1.0 / alpha
    omegaprod = 2.0 / alpha
    ckm1, ck = 1.0, mu
    out = []
    for _ in range(1, nsteps):
        ckp1 = 2.0 * mu * ck - ckm1
        omega = omegaprod * ck / ckp1
        out.append((1.0 - omega, omega, omega * Gamma * scale))
        ckm1, ck = ck, ckp1
    return scale, out


def cheb7(emin, emax):
    """the seven doubles the mgk_cheby3_2d_* entry points take"""
    s, c = cheb_steps(emin, emax, 3)
    return np.array([s, *c[0], *c[1]], dtype=np.float64)


def ksp_solve(orc, dim, n, As, b, u, steps, emin, emax, zero):
    """KSPSolve(max_it = steps) on a constant stencil: the first step is always taken (PETSc's cheby.c; oracle/mgo.c)"""
    s, c = cheb_steps(emin, emax, max(steps, 1))
    pkm1 = np.zeros_like(b) if zero else u
    pk = orc.jacobi(dim, n, As, s, b, pkm1, zero_guess=zero)
    for a, w, g in c:
        pkm1, pk = pk, orc.cheby_step(dim, n, As, b, pk, pkm1, a, w, g)
    return pk


def ksp_solve_rt(ct, dt, b, u, steps, emin, emax, zero):
    """the same on a 2-D row-table operator, in the canonical term order (tests/row_tables.py); b, u: (n, n)"""
    s, c = cheb_steps(emin, emax, max(steps, 1))
    pkm1 = np.zeros_like(b) if zero else u
    pk = s * (b * dt[:, None]) if zero else _rt_jacobi(ct, b, pkm1, s)
    for a, w, g in c:
        z = (b - _rt_apply(ct, pk)) * dt[:, None]
        pkm1, pk = pk, (a * pkm1 + w * pk) + g * z
    return pk
