"""Full multigrid (tests/fmg_reference.py) on the CPU oracle alone: the restatement is tied to the oracle's own V-cycle, and FMG(1) really
reaches the discretisation error.  No GPU."""
import numpy as np
import pytest

from fmg_reference import FmgRef
from oracle import Oracle

# (dim, npts, levels, scale): the sizes of the issue, V(3,3)
CASES = [(2, 129, 7, 0.8), (2, 257, 8, 0.8), (3, 33, 5, 6.0 / 7.0), (3, 65, 6, 6.0 / 7.0)]
# max-norm error of FMG(1) over that of the converged solution (the discretisation error), measured with this file's code:
# 2-D 129^2 1.660, 257^2 1.738; 3-D 33^3 5.956, 65^3 7.539 (Jacobi with scale 6/7 is a weaker smoother in 3-D).  Bounds: ~15-20 % above
RATIO_BOUND = {2: 2.0, 3: 9.0}


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("dim,npts,levels,scale", [(2, 33, 4, 0.8), (2, 65, 6, 0.8), (3, 17, 3, 6.0 / 7.0), (3, 33, 5, 6.0 / 7.0)])
@pytest.mark.parametrize("v", [(3, 3), (2, 1)])
def test_rooted_cycle_from_zero_equals_the_oracle_cycle(orc, dim, npts, levels, scale, v):
    """the helper's V-cycle rooted at level 0 from the zero guess, k times, equals Oracle.vcycle(fixed_cycles=k) bit for bit"""
    f = FmgRef(orc, dim, npts, levels, v, scale)
    k = 3
    u = f.vcycle(0, f.b0, None, nonzero=False)
    for _ in range(k - 1):
        u = f.vcycle(0, f.b0, u)
    ref = orc.vcycle(dim, npts, levels, v[0], v[1], maxiter=k, scale=scale, fixed_cycles=k)
    assert ref["iters"] == k
    assert np.array_equal(u, ref["u"])
    assert abs(f.rnorm_of(u) / ref["rnorm"][k] - 1.0) <= 1e-12


def _fmg_error(orc, dim, npts, levels, scale):
    f = FmgRef(orc, dim, npts, levels, (3, 3), scale)
    return orc.error_norms(dim, npts, f.fmg(1))[0]


@pytest.mark.parametrize("dim,npts,levels,scale", CASES)
def test_fmg1_reaches_the_discretisation_error(orc, dim, npts, levels, scale):
    efmg = _fmg_error(orc, dim, npts, levels, scale)
    conv = orc.vcycle(dim, npts, levels, 3, 3, maxiter=200, scale=scale, rtol=1e-12)
    edisc = orc.error_norms(dim, npts, conv["u"])[0]
    assert conv["iters"] < 200
    assert efmg <= RATIO_BOUND[dim] * edisc, (efmg, edisc, efmg / edisc)
    # ... and one V-cycle from zero is far from it: FMG is what gets there
    f = FmgRef(orc, dim, npts, levels, (3, 3), scale)
    e1 = orc.error_norms(dim, npts, f.vcycle(0, f.b0, None, nonzero=False))[0]
    assert e1 > 2 * efmg, (e1, efmg)


def test_fmg1_keeps_second_order(orc):
    """halving h divides the FMG(1) error by about four (2-D 129^2 -> 257^2: 3.82 measured)"""
    e129 = _fmg_error(orc, 2, 129, 7, 0.8)
    e257 = _fmg_error(orc, 2, 257, 8, 0.8)
    assert 3.5 <= e129 / e257 <= 4.5, e129 / e257


def test_solve_fmg_needs_fewer_cycles(orc):
    """FMG(1) + V-cycles to rtol 1e-7 take fewer iterations than V-cycles from zero (FMG counting as one)"""
    for dim, npts, levels, scale in CASES:
        f = FmgRef(orc, dim, npts, levels, (3, 3), scale)
        it, u, rn = f.solve_fmg(1, maxiter=100, rtol=1e-7)
        plain = orc.vcycle(dim, npts, levels, 3, 3, maxiter=100, scale=scale)
        assert rn[-1] <= 1e-7 * f.bnorm() and len(rn) == it + 1
        assert it < plain["iters"], (dim, npts, it, plain["iters"])


def test_the_fmg_entry_points_are_built_and_kept_out_of_the_mock_linked_host_code():
    """mg_solver_fmg / mg_solver_solve_fmg and the three FMG kernels are declared and exported; the host code that the CPU tier links
    against tests/mock_mgk.cpp (mg_solver.c and the rest) never names them -- only mg_fmg.c does"""
    import ctypes
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "multigrid_petsc_amd")
    kern = ("mgk_interp_jacobi2_f64", "mgk_interp_jacobi2_ok_f64", "mgk_interp_jacobi3_2d_f64", "mgk_tail_fmg_f64")
    api = ("mg_solver_fmg", "mg_solver_solve_fmg")
    hk, hs = open(os.path.join(root, "include", "mgk.h")).read(), open(os.path.join(root, "include", "mgsolve.h")).read()
    assert all(k + "(" in hk for k in kern) and all(a + "(" in hs for a in api)
    Lk = ctypes.CDLL(os.path.join(lib, "libmgk.so"))
    Lp = ctypes.CDLL(os.path.join(lib, "libmgpetsc.so"))
    assert all(hasattr(Lk, k) for k in kern) and all(hasattr(Lp, a) for a in api)
    csrc = os.path.join(lib, "csrc")
    for f in ("mg_solver.c", "mg_comm.c", "petsc_shim.c", os.path.join("driver", "mgpoisson.c")):
        text = open(os.path.join(csrc, f)).read()
        for name in kern + api:
            assert name not in text, f"{f} names {name}"
