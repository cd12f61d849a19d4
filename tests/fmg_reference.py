"""Full multigrid FMG(nu) and the V-cycles that follow it, restated from the CPU oracle's step primitives (Oracle.restrict, prolong_add onto
zeros, jacobi, residual, sumsq) in the order of mg_solver_fmg / mg_solver_solve_fmg (include/mgsolve.h).  Test infrastructure only.

  b_l = R b_{l-1} (l = 1 .. L-1);  u_{L-1} = v1 sweeps on b_{L-1} from the zero guess;
  for l = L-2 .. 0:  u_l = 0 + P u_{l+1}, then nu V-cycles on the levels l .. L-1 from that guess -- level l in the role of level 0 of
  the reference's loop (src/solver.c:1531-1543): v0 sweeps from the guess, residual + restriction + zero-guess sweeps down (v1 on the
  coarsest), prolongation + v0 sweeps up."""
import numpy as np


class FmgRef:
    def __init__(self, orc, dim, npts, levels, v=(3, 3), scale=1.0, b0=None):
        self.orc, self.dim, self.levels, self.v, self.scale = orc, dim, levels, tuple(v), scale
        self.n = [(npts - 1) // (1 << l) - 1 for l in range(levels)]
        self.As = [orc.level_stencil(dim, npts, l)[0] for l in range(levels)]
        self.b0 = orc.rhs(dim, npts) if b0 is None else np.ascontiguousarray(b0, dtype=np.float64)

    def zeros(self, l):
        return np.zeros(self.n[l] ** self.dim)

    def restrict(self, l, r):                  # level l -> l + 1
        return self.orc.restrict(self.dim, self.n[l], r)

    def prolong_add(self, l, uc, u):           # u_l + P u_{l+1}
        return self.orc.prolong_add(self.dim, self.n[l], uc, u)

    def residual(self, l, b, u):
        return self.orc.residual(self.dim, self.n[l], self.As[l], b, u)

    def smooth(self, l, b, u, sweeps, nonzero):
        """KSPSolve with `sweeps` Richardson + Jacobi sweeps; from the zero guess unless nonzero"""
        cur = u if nonzero else self.zeros(l)
        for it in range(sweeps):
            zg = (it == 0 and not nonzero)
            cur = self.orc.jacobi(self.dim, self.n[l], self.As[l], self.scale, b, cur, zero_guess=zg)
        return cur

    def vcycle(self, l, b, u, nonzero=True):
        """one V-cycle on the levels l .. L-1 from the guess u (the zero guess when nonzero is False); returns the new u_l"""
        L, (v0, v1) = self.levels, self.v
        if l == L - 1:
            return self.smooth(l, b, u, v1, nonzero)
        bs, us = {l: b}, {l: self.smooth(l, b, u, v0, nonzero)}
        for q in range(l + 1, L):
            bs[q] = self.restrict(q - 1, self.residual(q - 1, bs[q - 1], us[q - 1]))
            us[q] = self.smooth(q, bs[q], None, v1 if q == L - 1 else v0, False)
        for q in range(L - 2, l - 1, -1):
            us[q] = self.smooth(q, bs[q], self.prolong_add(q, us[q + 1], us[q]), v0, True)
        return us[l]

    def fmg(self, nu=1):
        L = self.levels
        bs = [self.b0]
        for l in range(1, L):
            bs.append(self.restrict(l - 1, bs[l - 1]))
        u = self.smooth(L - 1, bs[L - 1], None, self.v[1], False)
        for l in range(L - 2, -1, -1):
            ul = self.prolong_add(l, u, self.zeros(l))
            for _ in range(nu):
                ul = self.vcycle(l, bs[l], ul)
            u = ul
        return u

    def rnorm_of(self, u):
        return float(np.sqrt(self.orc.sumsq(self.residual(0, self.b0, u))))

    def bnorm(self):
        return float(np.sqrt(self.orc.sumsq(self.b0)))

    def fmg_then_cycles(self, nu, k):
        """FMG(nu) and k V-cycles: (u, rnorm[0 .. k+1])"""
        u = self.fmg(nu)
        rn = [self.rnorm_of(self.zeros(0)), self.rnorm_of(u)]
        for _ in range(k):
            u = self.vcycle(0, self.b0, u)
            rn.append(self.rnorm_of(u))
        return u, np.array(rn)

    def solve_fmg(self, nu, maxiter=1000, rtol=1e-7):
        """FMG(nu) as iteration 1, then V-cycles under the stop rule of src/solver.c:1530: (iterations, u, rnorm)"""
        bnorm = self.bnorm()
        u = self.fmg(nu)
        rn = [self.rnorm_of(self.zeros(0)), self.rnorm_of(u)]
        it = 1
        while it < maxiter and 100000000 * bnorm > rn[-1] and rn[-1] > rtol * bnorm:
            u = self.vcycle(0, self.b0, u)
            rn.append(self.rnorm_of(u))
            it += 1
        return it, u, np.array(rn)
