"""KSPCHEBYSHEV on the fused cycle (fuse bit 15) through Solver, against the CPU oracle's V-cycle with its Chebyshev smoother
(Oracle.vcycle(ksp_type=1)): same iteration count, residual history to 1e-12, solution bit for bit.  2-D: three-step passes on every
launched level, the Chebyshev tail kernel, the coarse-level graph; 3-D: the tail kernel alone.  The default mask against bit 15 off (the
step-by-step path, the reference of this work) bit for bit.  Reference: src/solver.c:1531-1546 with KSPCHEBYSHEV, max_it = v0 / v1."""
import numpy as np
import pytest

from oracle import Oracle

pytestmark = pytest.mark.gpu
RTOL = 1e-12
EIG = (0.2, 2.0)
DEFAULT = 63 | 0xFF00                         # bits 0-5 and 8-15
OFF15 = DEFAULT & ~32768


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _solver(dim, npts, levels, v=(3, 3), fuse=-1, mesh=0, maxiter=100, eig=EIG):
    from multigrid_petsc_amd.solver import Solver
    s = Solver(dim, npts, levels, v=v, maxiter=maxiter, ksp_type="chebyshev", eigenvalues=eig, fuse=fuse, mesh=mesh)
    s.set_rhs_problem()
    return s


def _ref(orc, dim, npts, levels, v=(3, 3), mesh=0, maxiter=100, fixed=0, eig=EIG):
    return orc.vcycle(dim, npts, levels, v[0], v[1], maxiter=maxiter, ksp_type=1, emin=eig[0], emax=eig[1], use_csr=1 if mesh else 0,
                      fixed_cycles=fixed, mesh=mesh)


def _full_depth(npts):
    return (npts - 1).bit_length() - 1


def _same(s, it, ref):
    assert it == ref["iters"], (it, ref["iters"])
    assert np.abs(s.rnorm / ref["rnorm"] - 1).max() <= RTOL
    assert np.array_equal(s.solution(), ref["u"])


@pytest.mark.parametrize("npts", [17, 65, 129, 257, 1025, 2049, 4097])
def test_2d_full_depth_equals_the_oracle(orc, npts):
    levels = _full_depth(npts)
    s = _solver(2, npts, levels)
    it = s.solve()
    ref = _ref(orc, 2, npts, levels)
    assert it < 100
    _same(s, it, ref)
    s.close()


@pytest.mark.parametrize("npts", [129, 1025])
@pytest.mark.parametrize("levels", [2, 3])
def test_2d_shallow_hierarchies_over_a_fixed_run(orc, npts, levels):
    """no tail, the coarsest level is a launched one (v1 = 3: a three-step pass from the zero guess): the graph stays off or is valid"""
    s = _solver(2, npts, levels)
    s.cycles(4)
    s.sync()
    ref = _ref(orc, 2, npts, levels, maxiter=4, fixed=4)
    _same(s, 4, ref)
    s.close()


@pytest.mark.parametrize("mesh", [1, 2])
@pytest.mark.parametrize("npts", [129, 257])
def test_2d_stretched_meshes_equal_the_assembled_leg(orc, mesh, npts):
    levels = _full_depth(npts)
    s = _solver(2, npts, levels, mesh=mesh, maxiter=300)
    it = s.solve()
    ref = _ref(orc, 2, npts, levels, mesh=mesh, maxiter=300)
    assert it < 300
    _same(s, it, ref)
    s.close()


@pytest.mark.parametrize("npts", [33, 65, 129])
def test_3d_tail_only_equals_the_oracle(orc, npts):
    levels = _full_depth(npts)
    s = _solver(3, npts, levels)
    it = s.solve()
    ref = _ref(orc, 3, npts, levels)
    assert it < 100
    _same(s, it, ref)
    s.close()


@pytest.mark.parametrize("dim,npts", [(2, 257), (2, 1025), (3, 65)])
@pytest.mark.parametrize("other", [OFF15, DEFAULT & ~512])
def test_default_mask_equals_the_unfused_paths_bit_for_bit(dim, npts, other):
    """bit 15 off (every step a launch), and bit 9 (the tail kernel) off with bit 15 on: the same solution bits over cycles(5) and over
    solve(), the same iteration count, the same history to 1e-12"""
    levels = _full_depth(npts)
    a, b = _solver(dim, npts, levels), _solver(dim, npts, levels, fuse=other)
    for s in (a, b):
        s.cycles(5)
        s.sync()
    # the fields bit for bit; the norms come out of different reduction kernels (the norm pass's per-wave partials against the residual +
    # norm kernel's per-block ones), so the histories agree as histories do everywhere: to 1e-12
    assert np.array_equal(a.solution(), b.solution())
    assert np.abs(a.rnorm / b.rnorm - 1).max() <= RTOL
    for s in (a, b):
        s.reset()
    ia, ib = a.solve(), b.solve()
    assert ia == ib and np.array_equal(a.solution(), b.solution())
    assert np.abs(a.rnorm / b.rnorm - 1).max() <= RTOL
    a.close()
    b.close()


@pytest.mark.parametrize("dim,npts", [(2, 257), (2, 1025), (3, 33)])
@pytest.mark.parametrize("v", [(3, 3), (3, 1), (2, 2), (4, 3)])
def test_step_counts(orc, dim, npts, v):
    """(3,3) and (3,1) take the three-step passes in 2-D; (2,2) and (4,3) must simply equal the oracle on the step-by-step path (above the
    tail, which takes any counts)"""
    levels = _full_depth(npts)
    s = _solver(dim, npts, levels, v=v, maxiter=200)
    it = s.solve()
    ref = _ref(orc, dim, npts, levels, v=v, maxiter=200)
    assert it < 200
    _same(s, it, ref)
    s.close()


@pytest.mark.parametrize("dim,npts", [(2, 513), (2, 2049), (3, 65)])
def test_solve_reset_solve_and_cycles_after_a_solve(orc, dim, npts):
    """graph replay from fresh state, adoption of the speculative pass, and stopping with a speculative pass outstanding"""
    levels = _full_depth(npts)
    s = _solver(dim, npts, levels)
    ref = _ref(orc, dim, npts, levels)
    it = s.solve()
    _same(s, it, ref)
    s.reset()
    it2 = s.solve()
    _same(s, it2, ref)
    # three more cycles from the converged state: the oracle with a tolerance it never reaches stops at the same count
    s.cycles(3)
    s.sync()
    more = orc.vcycle(dim, npts, levels, 3, 3, maxiter=it + 3, ksp_type=1, emin=EIG[0], emax=EIG[1], fixed_cycles=it + 3)
    assert s.iterations == it + 3
    assert np.abs(s.rnorm[:it + 1] / ref["rnorm"] - 1).max() <= RTOL
    assert np.array_equal(s.solution(), more["u"])
    assert np.abs(s.rnorm / more["rnorm"] - 1).max() <= RTOL
    s.close()


@pytest.mark.parametrize("eig", [(0.5, 2.0), (0.05, 1.7)])
def test_other_eigenvalue_bounds(orc, eig):
    s = _solver(2, 513, 9, eig=eig, maxiter=300)
    it = s.solve()
    ref = _ref(orc, 2, 513, 9, eig=eig, maxiter=300)
    _same(s, it, ref)
    s.close()
