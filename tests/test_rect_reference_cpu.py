"""tests/rect_reference.py, the numpy reference of the 2-D kernels on rectangles, pinned before tests/test_rect2d_gpu.py leans on it.
On squares each of its six operations equals the CPU oracle's bits (apply, residual, sweep, Chebyshev step, full weighting, prolongation-and-add)
and, on row tables, tests/row_tables.py; on a rectangle, swapping W with E or S with N in distinct coefficients changes the result, and the
transfers are held to their definitions point by point."""
import numpy as np
import pytest

import rect_reference as RR
from cheby_reference import cheb7, ksp_solve, ksp_solve_rt
from coef_cases import dense_field, distinct_coef, distinct_row_tables
from oracle import Oracle
from row_tables import _rt_apply, _rt_jacobi

SC = 6.0 / 7.0
CHEB = (-0.37, 1.37, 0.21)
EIG = (0.5, 2.0)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("n", [7, 15, 63])
def test_squares_equal_the_oracle_bit_for_bit(orc, n):
    rng = np.random.default_rng(91000 + n)
    nc = (n - 1) // 2
    As = distinct_coef(rng, 2)
    ct, dt = RR.const_table(As, n)
    u, b, pm, uc = dense_field(rng, n, n), dense_field(rng, n, n), dense_field(rng, n, n), dense_field(rng, nc, nc)
    f = lambda a: np.ascontiguousarray(a).ravel()
    assert np.array_equal(f(RR.apply(ct, u)), orc.apply(2, n, As, f(u)))
    assert np.array_equal(f(RR.residual(ct, b, u)), orc.residual(2, n, As, f(b), f(u)))
    for s in (SC, 0.8, 1.0):
        assert np.array_equal(f(RR.sweep(ct, dt, s, b, u)), orc.jacobi(2, n, As, s, f(b), f(u)))
        assert np.array_equal(f(RR.sweep_zero(dt, s, b)), orc.jacobi(2, n, As, s, f(b), np.zeros(n * n), zero_guess=True))
    assert np.array_equal(f(RR.cheby_step(ct, dt, b, u, pm, *CHEB)), orc.cheby_step(2, n, As, f(b), f(u), f(pm), *CHEB))
    assert np.array_equal(f(RR.restrict(u)), orc.restrict(2, n, f(u)))
    assert np.array_equal(f(RR.prolong_add(uc, u)), orc.prolong_add(2, n, f(uc), f(u)))
    assert np.array_equal(f(RR.prolong_add(uc, np.zeros((n, n)))), orc.prolong_add(2, n, f(uc), np.zeros(n * n)))
    c7 = cheb7(*EIG)
    assert np.array_equal(f(RR.cheby3(ct, dt, c7, b, u)), ksp_solve(orc, 2, n, As, f(b), f(u), 3, *EIG, zero=False))
    assert np.array_equal(f(RR.cheby3(ct, dt, c7, b, None)), ksp_solve(orc, 2, n, As, f(b), None, 3, *EIG, zero=True))


@pytest.mark.parametrize("n", [7, 15, 63])
def test_row_tables_on_squares_equal_row_tables_py(n):
    rng = np.random.default_rng(92000 + n)
    ct, dt = distinct_row_tables(rng, n)
    u, b = dense_field(rng, n, n), dense_field(rng, n, n)
    assert np.array_equal(RR.apply(ct, u), _rt_apply(ct, u))
    assert np.array_equal(RR.sweep(ct, dt, SC, b, u), _rt_jacobi(ct, b, u, SC))
    c7 = cheb7(*EIG)
    assert np.array_equal(RR.cheby3(ct, dt, c7, b, u), ksp_solve_rt(ct, dt, b, u, 3, *EIG, zero=False))
    assert np.array_equal(RR.cheby3(ct, dt, c7, b, None), ksp_solve_rt(ct, dt, b, None, 3, *EIG, zero=True))


@pytest.mark.parametrize("ny,nx", [(5, 119), (119, 7), (13, 243), (37, 63)])
def test_a_swapped_pair_of_coefficients_changes_the_result_on_a_rectangle(ny, nx):
    rng = np.random.default_rng(93000 + nx)
    u, b = dense_field(rng, ny, nx), dense_field(rng, ny, nx)
    As = distinct_coef(rng, 2)
    tabs = [RR.const_table(As, ny), distinct_row_tables(rng, ny)]
    for ct, dt in tabs:
        base = RR.sweep(ct, dt, SC, b, u)
        for p, q in ((1, 3), (0, 4)):                       # W <-> E, S <-> N
            sw = ct.copy()
            sw[:, [p, q]] = ct[:, [q, p]]
            assert not np.array_equal(RR.apply(sw, u), RR.apply(ct, u)), (p, q)
            assert not np.array_equal(RR.sweep(sw, dt, SC, b, u), base), (p, q)
    # the operator point by point, written out with scalars in the canonical order
    ct, dt = tabs[1]
    au = RR.apply(ct, u)
    at = lambda i, j: u[i, j] if 0 <= i < ny and 0 <= j < nx else 0.0
    for i, j in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (ny // 2, nx // 2), (1, nx - 2)):
        t = ct[i, 0] * at(i - 1, j)
        t = t + ct[i, 1] * at(i, j - 1)
        t = t + ct[i, 2] * at(i, j)
        t = t + ct[i, 3] * at(i, j + 1)
        t = t + ct[i, 4] * at(i + 1, j)
        assert au[i, j] == t


@pytest.mark.parametrize("ny,nx", [(5, 119), (119, 7), (13, 243), (37, 63), (1, 3), (3, 1)])
def test_transfers_on_rectangles_point_by_point(ny, nx):
    rng = np.random.default_rng(94000 + nx + ny)
    nyc, nxc = RR.coarse_shape(ny, nx)
    rf, uf, uc = dense_field(rng, ny, nx), dense_field(rng, ny, nx), dense_field(rng, nyc, nxc)
    bc = RR.restrict(rf)
    assert bc.shape == (nyc, nxc)
    for ic in range(nyc):
        for jc in range(nxc):
            s = 0.0
            for di in range(3):
                for dj in range(3):
                    s += RR.W_RESTRICT[di, dj] * rf[2 * ic + di, 2 * jc + dj]
            assert bc[ic, jc] == s
    pu = RR.prolong_add(uc, uf)
    for i in range(ny):
        for j in range(nx):
            ics = [(i - 1) // 2] if i & 1 else [i // 2 - 1, i // 2]
            jcs = [(j - 1) // 2] if j & 1 else [j // 2 - 1, j // 2]
            s = 0.0
            for ic in ics:
                for jc in jcs:
                    if 0 <= ic < nyc and 0 <= jc < nxc:
                        s += ((1.0 if i & 1 else 0.5) * (1.0 if j & 1 else 0.5)) * uc[ic, jc]
            assert pu[i, j] == uf[i, j] + s
