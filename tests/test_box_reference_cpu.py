"""tests/box_reference.py, the numpy reference of the 3-D kernels on boxes, pinned before tests/test_box3d_gpu.py leans on it.  Each of its six
operations (sweep, zero-guess sweep, residual, Chebyshev step, full weighting, prolongation-and-add) equals the CPU oracle's bits: the fp64 forms
on cubes and on nz != n (the oracle's fp64 3-D operators take nx = ny), the fp32 forms on the oracle's thin entry points with ny and nz != n.  On a
box with three different extents a swapped pair of coefficients changes the result, and the operator and the transfers are held to their
definitions point by point."""
import numpy as np
import pytest

import box_reference as BR
from coef_cases import dense_field, distinct_coef, np_apply
from oracle import Oracle

SC = 6.0 / 7.0
CHEB = (-0.37, 1.37, 0.21)
POW2 = np.array([2.0, -4.0, 1.0, -16.0, -2.0, 8.0, -1.0])          # six off-diagonals +-2^e: the set of the exact-FMA instances


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _f(a):
    return np.ascontiguousarray(a).ravel()


@pytest.mark.parametrize("n,nz", [(7, 7), (23, 23), (7, 5), (11, 3), (11, 23), (15, 7)])
def test_fp64_equals_the_oracle_bit_for_bit(orc, n, nz):
    rng = np.random.default_rng(97000 + 100 * n + nz)
    nc, nzc = (n - 1) // 2, (nz - 1) // 2
    u, b, pm = (dense_field(rng, nz, n, n) for _ in range(3))
    uc = dense_field(rng, nzc, nc, nc)
    for As in (distinct_coef(rng, 3), POW2):
        assert np.array_equal(_f(BR.apply(As, u)), orc.apply(3, n, As, _f(u), nz=nz))
        assert np.array_equal(BR.apply(As, u), np_apply(As, u))
        assert np.array_equal(_f(BR.residual(As, b, u)), orc.residual(3, n, As, _f(b), _f(u), nz=nz))
        for s in (SC, 0.8, 1.0):
            assert np.array_equal(_f(BR.sweep(As, s, b, u)), orc.jacobi(3, n, As, s, _f(b), _f(u), nz=nz))
            assert np.array_equal(_f(BR.sweep_zero(As, s, b)), orc.jacobi(3, n, As, s, _f(b), np.zeros(u.size), zero_guess=True, nz=nz))
        assert np.array_equal(_f(BR.cheby_step(As, b, u, pm, *CHEB)), orc.cheby_step(3, n, As, _f(b), _f(u), _f(pm), *CHEB, nz=nz))
    assert np.array_equal(_f(BR.restrict(u)), orc.restrict(3, n, _f(u), nzf=nz, nzc=nzc))
    assert np.array_equal(_f(BR.prolong_add(uc, u)), orc.prolong_add(3, n, _f(uc), _f(u), nzf=nz, nzc=nzc))
    assert np.array_equal(_f(BR.prolong_add(uc, np.zeros_like(u))), orc.prolong_add(3, n, _f(uc), np.zeros(u.size), nzf=nz, nzc=nzc))


@pytest.mark.parametrize("nx,ny,nz", [(7, 7, 7), (11, 7, 5), (23, 5, 11), (47, 11, 7), (7, 23, 3)])
def test_fp32_equals_the_oracles_thin_forms_bit_for_bit(orc, nx, ny, nz):
    rng = np.random.default_rng(98000 + 100 * nx + 10 * ny + nz)
    nzc, nyc, nxc = BR.coarse_shape(nz, ny, nx)
    f32 = lambda *s: dense_field(rng, *s).astype(np.float32)
    u, b, uc = f32(nz, ny, nx), f32(nz, ny, nx), f32(nzc, nyc, nxc)
    for As in (distinct_coef(rng, 3), POW2):
        for s in (SC, 0.8):
            got = BR.sweep(As, s, b, u)
            assert got.dtype == np.float32
            assert np.array_equal(_f(got), orc.jacobi32(nx, As, s, _f(b), _f(u), nz=nz, ny=ny))
            assert np.array_equal(_f(BR.sweep_zero(As, s, b)), orc.jacobi32(nx, As, s, _f(b), _f(u), zero_guess=True, nz=nz, ny=ny))
        assert np.array_equal(_f(BR.residual(As, b, u)), orc.residual32(nx, As, _f(b), _f(u), nz=nz, ny=ny))
    assert np.array_equal(_f(BR.restrict(u)), orc.restrict32(nx, _f(u), nzf=nz, nzc=nzc, nyf=ny))
    assert np.array_equal(_f(BR.prolong_add(uc, u)), orc.prolong_add32(nx, _f(uc), _f(u), nzf=nz, nzc=nzc, nyf=ny))


@pytest.mark.parametrize("nx,ny,nz", [(11, 7, 5), (23, 5, 11)])
def test_a_swapped_pair_of_coefficients_changes_the_result_on_a_box(nx, ny, nz):
    rng = np.random.default_rng(99000 + nx)
    u, b = dense_field(rng, nz, ny, nx), dense_field(rng, nz, ny, nx)
    As = distinct_coef(rng, 3)
    base = BR.sweep(As, SC, b, u)
    for p, q in ((2, 4), (1, 5), (0, 6), (0, 1), (1, 2)):
        sw = As.copy()
        sw[[p, q]] = As[[q, p]]
        assert not np.array_equal(BR.sweep(sw, SC, b, u), base), (p, q)
    au = BR.apply(As, u)
    at = lambda k, i, j: u[k, i, j] if 0 <= k < nz and 0 <= i < ny and 0 <= j < nx else 0.0
    for k, i, j in ((0, 0, 0), (nz - 1, ny - 1, nx - 1), (0, ny - 1, 0), (nz - 1, 0, nx - 1), (nz // 2, ny // 2, nx // 2), (1, ny - 2, nx - 2)):
        t = As[0] * at(k - 1, i, j)
        t = t + As[1] * at(k, i - 1, j)
        t = t + As[2] * at(k, i, j - 1)
        t = t + As[3] * at(k, i, j)
        t = t + As[4] * at(k, i, j + 1)
        t = t + As[5] * at(k, i + 1, j)
        t = t + As[6] * at(k + 1, i, j)
        assert au[k, i, j] == t


@pytest.mark.parametrize("nx,ny,nz", [(11, 7, 5), (7, 5, 11), (3, 1, 1), (1, 3, 5)])
def test_transfers_on_boxes_point_by_point(nx, ny, nz):
    rng = np.random.default_rng(99500 + nx + 10 * ny)
    nzc, nyc, nxc = BR.coarse_shape(nz, ny, nx)
    rf, uf, uc = dense_field(rng, nz, ny, nx), dense_field(rng, nz, ny, nx), dense_field(rng, nzc, nyc, nxc)
    bc = BR.restrict(rf)
    assert bc.shape == (nzc, nyc, nxc)
    for kc in range(nzc):
        for ic in range(nyc):
            for jc in range(nxc):
                s = 0.0
                for dk in range(3):
                    for di in range(3):
                        for dj in range(3):
                            s += (BR.W1[dk] * BR.W2[di][dj]) * rf[2 * kc + dk, 2 * ic + di, 2 * jc + dj]
                assert bc[kc, ic, jc] == s
    pu = BR.prolong_add(uc, uf)
    par = lambda f: [(f - 1) // 2] if f & 1 else [f // 2 - 1, f // 2]
    wt = lambda f: 1.0 if f & 1 else 0.5
    for k in range(nz):
        for i in range(ny):
            for j in range(nx):
                s = 0.0
                for kc in par(k):
                    for ic in par(i):
                        for jc in par(j):
                            if 0 <= kc < nzc and 0 <= ic < nyc and 0 <= jc < nxc:
                                s += (wt(k) * (wt(i) * wt(j))) * uc[kc, ic, jc]
                assert pu[k, i, j] == uf[k, i, j] + s
