"""mg_fuse_bits by name on the GPU: a solve with fuse = Fuse.DEFAULT is the solve of fuse = -1, bit for bit -- at the smallest shapes where the
coarse-level graph, the LDS tail and levels with launches of their own all run (2-D: levels of 127, 63, .. unknowns per side; 3-D: 63, 31, 15, ..)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dim,npts,levels,scale", [(2, 129, 6, 0.8), (3, 65, 5, 6.0 / 7.0)])
def test_default_mask_by_name_equals_minus_one(dim, npts, levels, scale):
    from multigrid_petsc_amd import Fuse
    from multigrid_petsc_amd.solver import Solver
    res = []
    for fuse in (-1, int(Fuse.DEFAULT)):
        s = Solver(dim, npts, levels, v=(3, 3), maxiter=100, scale=scale, fuse=fuse)
        s.set_rhs_problem()
        it = s.solve()
        res.append((it, s.rnorm, s.solution()))
        s.close()
    (it0, rn0, u0), (it1, rn1, u1) = res
    assert it0 == it1 and 2 <= it0 < 100
    assert np.array_equal(rn0, rn1)
    assert np.array_equal(u0, u1)
