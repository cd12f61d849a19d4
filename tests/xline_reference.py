"""x-line Jacobi and the alternating line cycle in numpy: the definition that mgk_xline_forward_f64 / mgk_xline_backward_f64
(csrc/mgk_xline.hip), the host table of csrc/mg_xline.c and the cycles of Solver(pc_type="xline" | "altline") are held to, operation for
operation.  Test infrastructure only; the y sweep, the hierarchy, the cycle loop and the comparison are those of tests/line_reference.py.

Level with n x n unknowns, row i with the coefficients {S, W, C, E, N}_i = ct[i, 0..4].  T_x = the x-tridiagonal part of A: in row i the
constant-band matrix (W_i, C_i, E_i).

  table    m_{i,0} = C_i, g_{i,0} = 1/m_{i,0};  j >= 1: l_{i,j} = W_i g_{i,j-1}, t = l_{i,j} E_i, m_{i,j} = C_i - t, g_{i,j} = 1/m_{i,j}
           l_{i,0} = 0;  q_{i,j} = E_i g_{i,j}
  sweep    r = b - A u                  the five terms in the order of _rt_apply; from the zero guess r = b and u is not read
           y_{i,0} = r_{i,0}, y_{i,j} = r_{i,j} - l_{i,j} y_{i,j-1};  z_{i,j} = y_{i,j} g_{i,j}
           e_{i,n-1} = z_{i,n-1}, e_{i,j} = z_{i,j} - q_{i,j} e_{i,j+1};  u'_{i,j} = u_{i,j} + s e_{i,j}; from the zero guess u' = s e

Every product and every sum is rounded on its own.  Python loops over columns, vectorised over rows.  Alternation: within one KSPSolve
(one smoothing of max_it sweeps, counted from 0 in every call) sweep k is a y-line sweep for even k and an x-line sweep for odd k."""
import numpy as np

import line_reference as LR
from line_reference import RTOL, SCALE, case_key, case_rhs, compare, margins, solve  # noqa: F401  (re-exported)
from row_tables import _rt_apply


def table(ct, ncols=None):
    """g (n x ncols) of the x-tridiagonal part of the row-table operator ct (n x 5)"""
    n = ct.shape[0]
    ncols = n if ncols is None else ncols
    g = np.zeros((n, ncols))
    g[:, 0] = 1.0 / ct[:, 2]
    for j in range(1, ncols):
        l = ct[:, 1] * g[:, j - 1]
        t = l * ct[:, 3]
        m = ct[:, 2] - t
        g[:, j] = 1.0 / m
    return g


def forward(ct, g, b, u=None):
    """z (n x n) of one sweep; u None: the zero guess"""
    n = b.shape[1]
    r = b if u is None else b - _rt_apply(ct, u)
    z = np.empty_like(b)
    y = r[:, 0].copy()
    z[:, 0] = y * g[:, 0]
    for j in range(1, n):
        l = ct[:, 1] * g[:, j - 1]
        t = l * y
        y = r[:, j] - t
        z[:, j] = y * g[:, j]
    return z


def backward(ct, g, scale, z, u=None):
    n = z.shape[1]
    out = np.empty_like(z)
    e = z[:, n - 1].copy()
    se = scale * e
    out[:, n - 1] = se if u is None else u[:, n - 1] + se
    for j in range(n - 2, -1, -1):
        q = ct[:, 3] * g[:, j]
        t = q * e
        e = z[:, j] - t
        se = scale * e
        out[:, j] = se if u is None else u[:, j] + se
    return out


def sweep(ct, g, scale, b, u=None):
    return backward(ct, g, scale, forward(ct, g, b, u), u)


class Hierarchy(LR.Hierarchy):
    """the level tables of one configuration and the smoothing of one pc_type ("yline", "xline", "altline")"""

    def __init__(self, orc, npts, levels, mesh, pc="altline"):
        super().__init__(orc, npts, levels, mesh)
        assert pc in ("yline", "xline", "altline")
        self.pc = pc
        self.xg = [table(ct) for ct in self.ct]
        self.log = []                                            # (level, "y" | "x") of every sweep, in order

    def smooth(self, l, scale, b, u, its):
        """KSPSolve with max_it = its; u None: from the zero guess.  Sweep k: y for even k, x for odd k (altline)"""
        if its == 0 and u is None:
            return np.zeros_like(b)
        for k in range(its):
            if self.pc == "yline" or (self.pc == "altline" and k % 2 == 0):
                u = LR.sweep(self.ct[l], self.tab[l], scale, b, u)
                self.log.append((l, "y"))
            else:
                u = sweep(self.ct[l], self.xg[l], scale, b, u)
                self.log.append((l, "x"))
        return u


# (pc, npts, levels, mesh, rhs, cycles): levels down to 1 x 1, V(3,3), scale 0.8, rtol 1e-7; rhs "manufactured" or "rough:<seed>"
# (tests/rhs_cases.uniform).  Every case has a stop decision clear of rounding on THIS reference (margins <= 0.8 and >= 1.5)
CASES = [("altline", 17, 4, 0, "manufactured", 7), ("altline", 17, 4, 1, "manufactured", 7), ("altline", 33, 5, 0, "manufactured", 7),
         ("altline", 33, 5, 1, "manufactured", 7), ("altline", 33, 5, 2, "manufactured", 8), ("altline", 65, 6, 0, "manufactured", 7),
         ("altline", 65, 6, 2, "manufactured", 8), ("altline", 129, 7, 0, "manufactured", 7), ("altline", 257, 8, 1, "manufactured", 8),
         ("altline", 17, 4, 2, "rough:1", 6), ("altline", 33, 5, 1, "rough:1", 6), ("altline", 65, 6, 2, "rough:1", 7),
         ("altline", 129, 7, 2, "rough:1", 7),
         ("xline", 17, 4, 0, "manufactured", 7), ("xline", 33, 5, 0, "manufactured", 7), ("xline", 65, 6, 0, "manufactured", 7),
         ("xline", 33, 5, 2, "manufactured", 12), ("xline", 33, 5, 1, "rough:4", 14)]
_REF = {}


def xcase_key(case):
    return ",".join(str(c) for c in case[:5])


def reference(orc, case, v=(3, 3)):
    """the reference solve of a case (its log of sweeps under "log"), computed once per process and never changed"""
    key = (case[:5], tuple(v))
    if key not in _REF:
        pc, npts, levels, mesh, rhs = case[:5]
        h = Hierarchy(orc, npts, levels, mesh, pc)
        r = solve(h, case_rhs(h, rhs), SCALE, v=tuple(v), rtol=RTOL, maxiter=100)
        r["log"] = list(h.log)
        _REF[key] = r
    return _REF[key]
