"""Conjugate gradients in fp64 preconditioned by the fp32 V-cycle of the mixed-precision iteration, in numpy over the CPU oracle: the definition
that mg_solver_solve_cg_mixed (csrc/mg_cg_mixed.c) is held to.  Test infrastructure only.

  M r   (double) Vcycle32((float) r) from the zero guess: Oracle.vcycle_mixed(fixed_cycles=1, b=r)["u"] -- the outer iteration's one step from
        u = 0 is u = 0 + (double) e, and its first residual is (float)(r - A 0) = (float) r
  A x   Oracle.apply with the level-0 stencil in fp64, the canonical order

The recurrence, the two orders of summation and the bars are those of tests/cg_reference.py: cg_reference.cg runs on MixedOperators, and a result
is judged by cg_reference.judge unchanged (its true residual needs A alone).  3-D only, like the fp32 cycle.  What the reference gives on the
CPU at rtol 1e-7 (steps; last / previous entry in units of rtol ||b||):
  converged   33^3 L4 0.8 rough:3   7   0.19 / 3.20        65^3 L5 0.8 rough:7   7   0.19 / 2.80
  off-width   25^3 L2 0.8 rough:2  15   0.56 / 2.58
  capped      33^3 L4 1.0 rough:4  30 to the tolerance (0.63 / 1.25: not clear of rounding), capped at 10
              17^3 L3 1.0 V(2,2) rough:1  19 to the tolerance (0.46 / 1.49), capped at 8
  breakdown   33^3 L4 1.5 rough:1  beta < 0 after the first completed update
The same counts as fp64 CG on every one of them; the fp32 cycle is symmetric to about 3e-7 only, which costs no step at this tolerance."""
import numpy as np

import cg_reference as R
from gmres_reference import Operators

CONVERGED = [
    (3, 33, 4, 0.8, (3, 3), "rough:3", 100),
    (3, 65, 5, 0.8, (3, 3), "rough:7", 100),
]
OFF_WIDTH = [(3, 25, 2, 0.8, (3, 3), "rough:2", 100)]
CAPPED = [                                          # scale 1: the stop margins are not clear of rounding, so the count is capped below it
    (3, 33, 4, 1.0, (3, 3), "rough:4", 10),
    (3, 17, 3, 1.0, (2, 2), "rough:1", 8),
]
BREAKDOWN = (3, 33, 4, 1.5, (3, 3), "rough:1", 100)
SCALE_ONE = (3, 33, 4, 1.0, (3, 3), "rough:4", 100)   # uncapped: 30 steps, where the plain mixed iteration is at 3.8e-5 ||b|| after 100 cycles
CASES = CONVERGED + OFF_WIDTH + CAPPED
# cg_reference.judge asks cg_reference.capped, which reads that module's list (tests/test_cg_solve_gpu.py extends it in the same way)
R.CAPPED.extend(c for c in CAPPED if c not in R.CAPPED)
key, parse, capped, judge, delta, distance, margins, cg = R.key, R.parse, R.capped, R.judge, R.delta, R.distance, R.margins, R.cg


class MixedOperators(Operators):
    """A in fp64 as in gmres_reference.Operators, M the one mixed cycle from the zero guess"""

    def __init__(self, orc, case):
        dim, npts, levels, scale, v, rhs, maxiter = case
        assert dim == 3
        super().__init__(orc, dim, npts, levels, 0, scale, v=v)

    def M(self, r):
        self.napply += 1
        return self.orc.vcycle_mixed(self.npts, self.levels, self.v[0], self.v[1], maxiter=1, scale=self.scale, fixed_cycles=1, b=r)["u"]


def reference(orc, case, rtol=1.0e-7):
    """(b, [the reference in the two orders of summation]) -- cg_reference.reference over the mixed operator"""
    op = MixedOperators(orc, case)
    b = R.rhs_of(op, case)
    refs = [R.cg(op, b, rtol=rtol, maxiter=case[6], dot=d) for d in ("np", "ld")]
    op.close()
    return b, refs


def asymmetry(orc, case, seed=5):
    """|a . M b - b . M a| / |a . M b| on random a, b"""
    op = MixedOperators(orc, case)
    rng = np.random.default_rng(seed)
    n = (case[1] - 2) ** 3
    a, b = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    aMb, bMa = float(np.dot(a, op.M(b))), float(np.dot(b, op.M(a)))
    op.close()
    return abs(aMb - bMa) / abs(aMb)
