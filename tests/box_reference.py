"""numpy statement of the 3-D level operations on BOXES (nz planes of ny rows of nx unknowns, all three extents allowed to differ): the reference of
tests/test_box3d_gpu.py, the 3-D twin of tests/rect_reference.py.  The CPU oracle's fp64 3-D operators take nx = ny; tests/test_box_reference_cpu.py
pins this module to them bit for bit on cubes and on nz != n, and to the oracle's fp32 thin forms on ny, nz != n.  Test infrastructure only.

 * the operator: seven constants As = {k-1, i-1, j-1, C, j+1, i+1, k+1} (the ABI's order, include/mgk.h), the seven products summed in that order over a
   field with a zero ghost shell; dinv = 1 / C
 * sweep, zero-guess sweep, residual, Chebyshev step: the expressions of include/mgk.h (mgk_jacobi_f64, mgk_jacobi_zero_f64, mgk_residual_f64,
   mgk_cheby_f64), every product and every sum rounded on its own (numpy does not contract)
 * full weighting: coarse (kc, ic, jc) gathers fine (2 kc + dk, 2 ic + di, 2 jc + dj), the 27 terms added in ascending fine index (dk, di, dj), each
   weight the exact product w1[dk] * (w2[di][dj])
 * prolongation-and-add: uf + P uc, the row of P summed over its parents in ascending coarse index (kc, ic, jc), weight wk * (wi * wj)
 * dtype = np.float32: the same expressions evaluated in binary32 on float32 arrays; the coefficients, 1 / C and the scale are the doubles rounded to
   float once (Oracle.coef32: (float) As[q], (float) (1 / As[3])), as the fp32 kernels take them"""
import numpy as np

W1 = (0.25, 0.5, 0.25)
W2 = ((0.0625, 0.125, 0.0625), (0.125, 0.25, 0.125), (0.0625, 0.125, 0.0625))


def _c(As, dtype):
    """(the seven coefficients, 1 / C) as scalars of dtype; 1 / C is formed in double and rounded once"""
    As = np.asarray(As, dtype=np.float64)
    assert As.shape == (7,)
    dt = np.dtype(dtype).type
    return [dt(a) for a in As], dt(1.0 / float(As[3]))


def _pad(x):
    p = np.zeros(tuple(s + 2 for s in x.shape), dtype=x.dtype)
    p[1:-1, 1:-1, 1:-1] = x
    return p


def apply(As, x):
    """A x, the seven terms in the order k-1, i-1, j-1, C, j+1, i+1, k+1"""
    assert x.ndim == 3 and x.dtype in (np.float64, np.float32)
    a, _ = _c(As, x.dtype)
    p = _pad(x)
    t = a[0] * p[:-2, 1:-1, 1:-1]
    t = t + a[1] * p[1:-1, :-2, 1:-1]
    t = t + a[2] * p[1:-1, 1:-1, :-2]
    t = t + a[3] * p[1:-1, 1:-1, 1:-1]
    t = t + a[4] * p[1:-1, 1:-1, 2:]
    t = t + a[5] * p[1:-1, 2:, 1:-1]
    t = t + a[6] * p[2:, 1:-1, 1:-1]
    assert t.dtype == x.dtype
    return t


def residual(As, b, u):
    return b - apply(As, u)


def sweep(As, scale, b, u):
    """u + scale * ((b - A u) * dinv)"""
    dt = u.dtype.type
    out = u + dt(scale) * (residual(As, b, u) * _c(As, u.dtype)[1])
    assert out.dtype == u.dtype
    return out


def sweep_zero(As, scale, b):
    """the sweep from the zero guess: scale * (b * dinv), u is not read"""
    dt = b.dtype.type
    return dt(scale) * (b * _c(As, b.dtype)[1])


def cheby_step(As, b, pk, pkm1, ckm1, ck, cz):
    """(c_km1 * pkm1 + c_k * pk) + c_z * ((b - A pk) * dinv)"""
    dt = pk.dtype.type
    return (dt(ckm1) * pkm1 + dt(ck) * pk) + dt(cz) * (residual(As, b, pk) * _c(As, pk.dtype)[1])


def coarse_shape(nz, ny, nx):
    assert nz % 2 == 1 and ny % 2 == 1 and nx % 2 == 1, "a vertex-centred level has an odd number of unknowns per axis"
    return (nz - 1) // 2, (ny - 1) // 2, (nx - 1) // 2


def restrict(rf):
    """full weighting onto the ((nz - 1) / 2, (ny - 1) / 2, (nx - 1) / 2) coarse grid"""
    nzc, nyc, nxc = coarse_shape(*rf.shape)
    dt = rf.dtype.type
    s = np.zeros((nzc, nyc, nxc), dtype=rf.dtype)
    for dk in range(3):
        for di in range(3):
            for dj in range(3):
                w = dt(W1[dk]) * dt(W2[di][dj])
                s = s + w * rf[dk:dk + 2 * nzc - 1:2, di:di + 2 * nyc - 1:2, dj:dj + 2 * nxc - 1:2]
    assert s.dtype == rf.dtype
    return s


def prolong_add(uc, uf):
    """uf + P uc: a fine point with an odd index on an axis has one parent there (weight 1), with an even index two (weight 1/2 each, the one
    outside the grid dropped: a zero of the padded array adds nothing)"""
    nzc, nyc, nxc = uc.shape
    assert uf.shape == (2 * nzc + 1, 2 * nyc + 1, 2 * nxc + 1) and uc.dtype == uf.dtype
    dt = uf.dtype.type
    p = _pad(uc)
    s = np.zeros_like(uf)
    # per axis and parity of the fine index: the slices of the padded coarse array that hold its parents, ascending, and their weight
    par = lambda n: {1: ([slice(1, n + 1)], 1.0), 0: ([slice(0, n + 1), slice(1, n + 2)], 0.5)}
    pk, pi, pj = par(nzc), par(nyc), par(nxc)
    for ek in (0, 1):
        for ei in (0, 1):
            for ej in (0, 1):
                (sk, wk), (si, wi), (sj, wj) = pk[ek], pi[ei], pj[ej]
                w = dt(wk) * (dt(wi) * dt(wj))
                t = np.zeros((len(range(ek, uf.shape[0], 2)), len(range(ei, uf.shape[1], 2)), len(range(ej, uf.shape[2], 2))), dtype=uf.dtype)
                for a in sk:
                    for b_ in si:
                        for c in sj:
                            t = t + w * p[a, b_, c]
                s[ek::2, ei::2, ej::2] = t
    out = uf + s
    assert out.dtype == uf.dtype
    return out
