"""numpy statement of the 2-D level operations on RECTANGULAR fields (ny rows of nx unknowns, nx != ny allowed): the reference of
tests/test_rect2d_gpu.py.  The CPU oracle's 2-D operators and tests/row_tables.py are square only; tests/test_rect_reference_cpu.py pins this
module to both, bit for bit, on squares.  Test infrastructure only.

 * the operator: per grid row i five coefficients ct[i] = {S, W, C, E, N} = {(i-1), (j-1), centre, (j+1), (i+1)} and dt[i] (1 / C_i on the levels
   of a solver), the five products summed in that order over a field with a zero ghost ring; a constant stencil is a table of equal rows
 * sweep, zero-guess sweep, residual, Chebyshev step: the expressions of include/mgk.h (mgk_jacobi_f64, mgk_jacobi_zero_f64, mgk_residual_f64,
   mgk_cheby_f64), every product and every sum rounded on its own (numpy does not contract)
 * full weighting: coarse (ic, jc) gathers fine (2 ic + di, 2 jc + dj), the nine terms added in ascending fine index (di, dj)
 * prolongation-and-add: uf + P uc, the row of P summed over its parents in ascending coarse index (ic, jc)"""
import numpy as np

W_RESTRICT = np.array([[0.0625, 0.125, 0.0625], [0.125, 0.25, 0.125], [0.0625, 0.125, 0.0625]])


def const_table(coef, ny):
    """the row tables of a constant five-point stencil {S, W, C, E, N}: (ct (ny, 5), dt (ny,) = 1 / C)"""
    coef = np.asarray(coef, dtype=np.float64)
    return np.tile(coef, (ny, 1)), np.full(ny, 1.0 / float(coef[2]))


def apply(ct, u):
    """A u, the five terms in the order S, W, C, E, N"""
    ny, nx = u.shape
    assert ct.shape == (ny, 5)
    p = np.zeros((ny + 2, nx + 2))
    p[1:-1, 1:-1] = u
    t = ct[:, 0:1] * p[:-2, 1:-1]
    t = t + ct[:, 1:2] * p[1:-1, :-2]
    t = t + ct[:, 2:3] * p[1:-1, 1:-1]
    t = t + ct[:, 3:4] * p[1:-1, 2:]
    t = t + ct[:, 4:5] * p[2:, 1:-1]
    return t


def residual(ct, b, u):
    return b - apply(ct, u)


def sweep(ct, dt, scale, b, u):
    """u + scale * ((b - A u) * dt_i)"""
    return u + scale * (residual(ct, b, u) * np.asarray(dt).reshape(-1, 1))


def sweep_zero(dt, scale, b):
    """the sweep from the zero guess: scale * (b * dt_i), u is not read"""
    return scale * (b * np.asarray(dt).reshape(-1, 1))


def cheby_step(ct, dt, b, pk, pkm1, ckm1, ck, cz):
    """(c_km1 * pkm1 + c_k * pk) + c_z * ((b - A pk) * dt_i)"""
    return (ckm1 * pkm1 + ck * pk) + cz * (residual(ct, b, pk) * np.asarray(dt).reshape(-1, 1))


def cheby3(ct, dt, cheb7, b, u):
    """KSPSolve with max_it = 3 of KSPCHEBYSHEV: cheb7 = {s, (c_km1, c_k, c_z) of step 2, of step 3} (tests/cheby_reference.py cheb7); u None:
    from the zero guess"""
    s = float(cheb7[0])
    pkm1 = np.zeros_like(b) if u is None else u
    pk = sweep_zero(dt, s, b) if u is None else sweep(ct, dt, s, b, u)
    for q in (1, 4):
        pkm1, pk = pk, cheby_step(ct, dt, b, pk, pkm1, float(cheb7[q]), float(cheb7[q + 1]), float(cheb7[q + 2]))
    return pk


def coarse_shape(ny, nx):
    assert ny % 2 == 1 and nx % 2 == 1, "a vertex-centred level has an odd number of unknowns per axis"
    return (ny - 1) // 2, (nx - 1) // 2


def restrict(rf):
    """full weighting onto the ((ny - 1) / 2, (nx - 1) / 2) coarse grid"""
    nyc, nxc = coarse_shape(*rf.shape)
    s = np.zeros((nyc, nxc))
    for di in range(3):
        for dj in range(3):
            s = s + W_RESTRICT[di, dj] * rf[di:di + 2 * nyc - 1:2, dj:dj + 2 * nxc - 1:2]
    return s


def prolong_add(uc, uf):
    """uf + P uc: a fine point with an odd index on an axis has one parent there (weight 1), with an even index two (weight 1/2 each, the one
    outside the grid dropped: a zero of the padded array adds nothing)"""
    nyc, nxc = uc.shape
    assert uf.shape == (2 * nyc + 1, 2 * nxc + 1)
    p = np.zeros((nyc + 2, nxc + 2))
    p[1:-1, 1:-1] = uc
    s = np.zeros_like(uf)
    s[1::2, 1::2] = 0.0 + (1.0 * 1.0) * uc
    t = 0.0 + (1.0 * 0.5) * p[1:-1, :-1]
    s[1::2, 0::2] = t + (1.0 * 0.5) * p[1:-1, 1:]
    t = 0.0 + (0.5 * 1.0) * p[:-1, 1:-1]
    s[0::2, 1::2] = t + (0.5 * 1.0) * p[1:, 1:-1]
    t = 0.0 + (0.5 * 0.5) * p[:-1, :-1]
    t = t + (0.5 * 0.5) * p[:-1, 1:]
    t = t + (0.5 * 0.5) * p[1:, :-1]
    s[0::2, 0::2] = t + (0.5 * 0.5) * p[1:, 1:]
    return uf + s
