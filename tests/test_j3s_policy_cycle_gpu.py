"""The load policy of the stacked 3-D pass inside a cycle: plain loads of b (the default) against the
non-temporal ones of TUNE_J3S_B_NT, inside one build.  The policy changes no value: solution and residual history are equal bit for bit.

npts = 513 is the smallest solver configuration whose cycle runs k_jacobi3s: the pass takes rows of 512 or 1024 only (jacobi3s_shape_ok() of
csrc/mgk_sweep3.hip; mg_solver.c asks mgk_jacobi3_mid_ok_f64 / mgk_prolong_jacobi3_ok_f64 per level), the solver's grids are cubes, and
level 0 of npts = 257 is 255 wide.  Fuse bit 17 is set (at rows of 512 it is opt-in), the right-hand side is a seeded random field, two
cycles in one call: the first cycle's prolongation + three-sweep pass and norm + three-sweep pass, the closing cycle's prolongation pass.
Both runs must have launched both passes."""
import numpy as np
import pytest

from multigrid_petsc_amd import FUSE_TRIPLE_MID, FUSE_TRIPLE_NORM, TUNE_J3S_B_NT, Fuse, tuning
from multigrid_petsc_amd.solver import Solver

pytestmark = pytest.mark.gpu

NPTS, LEVELS, SCALE = 513, 9, 6.0 / 7.0
FUSE = int(Fuse.DEFAULT) | FUSE_TRIPLE_MID | FUSE_TRIPLE_NORM


def _run(variant, rhs):
    with tuning(variant):
        s = Solver(3, NPTS, LEVELS, v=(3, 3), scale=SCALE, device=0, fuse=FUSE, maxiter=10)
        try:
            s.set_rhs(rhs)
            s.cycles(2)
            s.sync()
            return {"it": s.iterations, "rn": s.rnorm.copy(), "u": s.solution(), "norm": s.triple_norm_launches, "pro": s.prolong_triple_launches(0)}
        finally:
            s.close()


def test_two_cycles_under_both_policies():
    rhs = np.random.default_rng(72000).uniform(-1.0, 1.0, (NPTS - 2) ** 3)
    new, old = _run(-1, rhs), _run(int(TUNE_J3S_B_NT), rhs)
    print(f"iterations {new['it']} / {old['it']}, residual history {new['rn']!r}; norm + three-sweep launches {new['norm']} / {old['norm']}, "
          f"prolongation + three-sweep launches on level 0 {new['pro']} / {old['pro']}")
    assert new["it"] == old["it"] == 2
    assert new["norm"] == old["norm"] == 1 and new["pro"] == old["pro"] == 2           # the stacked passes ran, in both
    assert np.all(np.isfinite(new["rn"])) and new["rn"][-1] < new["rn"][0]
    assert np.array_equal(new["rn"], old["rn"]), (new["rn"], old["rn"])
    assert np.array_equal(new["u"], old["u"]), f"{np.count_nonzero(new['u'] != old['u'])} unknowns differ"
