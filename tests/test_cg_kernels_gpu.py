"""The two fused passes of the CG driver (csrc/mgk_cg.hip, include/mgk_cg.h) on random fields, under guarded.Guarded(mgk, poison=True): guard zones
round every buffer, poisoned outputs, a zero frame.

  mgk_cg_direction_apply_dot_f64   p_new = z + beta * p_old (first step: z), q = A p_new, sigma = p_new . q
  mgk_cg_update_sumsq_f64          x += alpha * p, r -= alpha * q, sum r^2

  field outputs   np.array_equal to the numpy expressions in the stated order (every product and sum rounded separately, A in the canonical order)
  sigma, sumsq    within 1e-13 relative of math.fsum over the rounded products (the bar of tests/test_gmres_kernels_gpu.py).  The coefficients are
                  distinct and non-symmetric (a swapped neighbour shows) with a dominant centre, so that sigma is well conditioned: the test
                  asserts sum |p_i (A p)_i| <= 4 |sigma| on its own inputs
  workspace       the partial slots are filled with NaN before EVERY call of the two passes: a slot that is summed and was not written turns
                  the sum into NaN.  The context's shared scratch is never used (tests/test_reduction_scratch_cpu.py scans for that)
  twice           the same call again gives the same bits
  interior only   Guarded: nothing outside the interiors is written, the guards are intact, every output cell is written
  forms           p_old = NULL with the poisoned p_new lying about, beta = 0 with a real p_old, both forced store policies at 127 x 127 and 31^3
  shapes          one lane, a half pair at the row end, one wave exactly, wave and block seams in x, strip seams in y, nx != ny != nz"""
import ctypes as C
import math

import numpy as np
import pytest

from cg_kernel_aids import capturing
from guarded import Guarded
from multigrid_petsc_amd.mgk import Geom, cg_sigs

pytestmark = pytest.mark.gpu
COEF2 = [-1.3, -0.7, 9.1, -1.1, -0.9]                       # {i-1, j-1, C, j+1, i+1}
COEF3 = [-0.6, -1.3, -0.7, 11.3, -1.1, -0.9, -0.8]          # {k-1, i-1, j-1, C, j+1, i+1, k+1}
SHAPES_2D = [(1, 1), (3, 5), (15, 15), (63, 63), (127, 127), (129, 3), (5, 131), (255, 7), (257, 5), (511, 3), (513, 3), (1023, 3)]
SHAPES_3D = [(1, 1, 1), (7, 7, 7), (31, 31, 31), (33, 5, 9), (9, 33, 5), (63, 63, 3), (129, 3, 3), (513, 3, 3)]
LARGE = [(4095, 4095), (1023, 1023, 3)]
CASES = [(s, -1) for s in SHAPES_2D + SHAPES_3D + LARGE] + [((127, 127), 0), ((127, 127), 1), ((31, 31, 31), 0), ((31, 31, 31), 1)]


def _id(c):
    return "x".join(str(n) for n in c[0]) + ("" if c[1] < 0 else f"-policy{c[1]}")


class Ws:
    """the reduction workspace of the two passes, and the NaN fill of its partial slots"""

    def __init__(self, mgk):
        self.mgk, self.p = mgk, C.c_void_p()
        cg_sigs(mgk.L)
        mgk._chk(mgk.L.mgk_cg_workspace_create(mgk.ctx, C.byref(self.p)))
        addr, n = C.c_void_p(), C.c_int()
        mgk._chk(mgk.L.mgk_cg_workspace_debug(self.p, C.byref(addr), C.byref(n)))
        assert addr.value and n.value >= 1024
        self.addr, self.n = addr, n.value
        self.nan = np.full(self.n, np.nan)

    def poison(self):
        self.mgk.sync()
        self.mgk._chk(self.mgk.L.mgk_h2d(self.mgk.ctx, self.addr, self.nan.ctypes.data_as(C.c_void_p), self.nan.nbytes))

    def slots(self):
        self.mgk.sync()
        return self.mgk.download(self.addr, self.n)

    def close(self):
        self.mgk.L.mgk_cg_workspace_destroy(self.mgk.ctx, self.p)


@pytest.fixture(scope="module")
def ws(mgk):
    w = Ws(mgk)
    yield w
    w.close()


def _apply(shape, coef, p):
    """A p in the canonical order on the zero-padded field, every product and sum rounded separately"""
    dims = shape[::-1]                                      # (nz,) ny, nx
    P = np.zeros(tuple(n + 2 for n in dims))
    P[tuple(slice(1, -1) for _ in dims)] = p.reshape(dims)
    if len(dims) == 2:
        t = coef[0] * P[:-2, 1:-1]
        t = t + coef[1] * P[1:-1, :-2]
        t = t + coef[2] * P[1:-1, 1:-1]
        t = t + coef[3] * P[1:-1, 2:]
        t = t + coef[4] * P[2:, 1:-1]
    else:
        t = coef[0] * P[:-2, 1:-1, 1:-1]
        t = t + coef[1] * P[1:-1, :-2, 1:-1]
        t = t + coef[2] * P[1:-1, 1:-1, :-2]
        t = t + coef[3] * P[1:-1, 1:-1, 1:-1]
        t = t + coef[4] * P[1:-1, 1:-1, 2:]
        t = t + coef[5] * P[1:-1, 2:, 1:-1]
        t = t + coef[6] * P[2:, 1:-1, 1:-1]
    return t.ravel()


def _close(got, exact):
    return abs(got - exact) <= 1e-13 * abs(exact)


def _direction(G, ws, g, coef, beta, z, p_old, pn, q):
    ws.poison()
    s = C.c_double()
    G._chk(G.L.mgk_cg_direction_apply_dot_f64(G.ctx, C.byref(g), G.coef(coef), beta, z, p_old, pn, q, ws.p, C.byref(s), None))
    return s.value


def _update(G, ws, g, alpha, p, q, x, r):
    ws.poison()
    s = C.c_double()
    G._chk(G.L.mgk_cg_update_sumsq_f64(G.ctx, C.byref(g), alpha, p, q, x, r, ws.p, C.byref(s), None))
    return s.value


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_the_two_passes(mgk, ws, case):
    shape, policy = case
    dim = len(shape)
    coef = COEF2 if dim == 2 else COEF3
    G = Guarded(mgk, poison=True)
    L = G.L
    g = G.geom(dim, *shape)
    N = int(np.prod(shape))
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + dim)
    zc, pc, xc, rc = (rng.uniform(-1, 1, N) for _ in range(4))
    beta, alpha = 0.37, 0.61
    L.mgk_set_tuning(policy, -1)
    try:
        big = N > 4000000                                   # the two large shapes: one call of each pass (every fetch moves the whole field)
        z, p_old, pn, q = G.to_field(g, zc), G.to_field(g, pc), G.field(g), G.field(g)
        if not big:
            # ---- the first step: p_new = z; the other buffers of the driver hold NaN (the poison) and must not reach the sum
            sig = _direction(G, ws, g, coef, beta, z, None, pn, q)
            q_ref = _apply(shape, coef, zc)
            assert np.array_equal(G.from_field(g, pn), zc) and np.array_equal(G.from_field(g, q), q_ref)
            assert _close(sig, math.fsum(zc * q_ref)), (sig, math.fsum(zc * q_ref))
            # ---- beta = 0 with a real p_old
            sig0 = _direction(G, ws, g, coef, 0.0, z, p_old, pn, q)
            assert np.array_equal(G.from_field(g, pn), zc + 0.0 * pc) and np.array_equal(G.from_field(g, q), q_ref) and sig0 == sig
        # ---- a later step
        sig = _direction(G, ws, g, coef, beta, z, p_old, pn, q)
        pn_ref = zc + beta * pc
        q_ref = _apply(shape, coef, pn_ref)
        exact = math.fsum(pn_ref * q_ref)
        assert math.fsum(np.abs(pn_ref * q_ref)) <= 4.0 * abs(exact)               # (a condition on the inputs: sigma is well conditioned)
        nblk = int(np.sum(~np.isnan(ws.slots())))
        assert 1 <= nblk <= ws.n
        assert np.array_equal(G.from_field(g, pn), pn_ref) and np.array_equal(G.from_field(g, q), q_ref)
        assert _close(sig, exact), (sig, exact)
        if not big:
            # the same call again: the same bits (the outputs were taken, so the proxy has poisoned them again)
            assert _direction(G, ws, g, coef, beta, z, p_old, pn, q) == sig
            assert np.array_equal(G.from_field(g, pn), pn_ref) and np.array_equal(G.from_field(g, q), q_ref)
            assert np.array_equal(G.from_field(g, z), zc) and np.array_equal(G.from_field(g, p_old), pc)      # the inputs are as they were
        for f in (z, p_old, pn, q):
            G.free(f)
        # ---- the update, in place (p and q as inputs of their own: the proxy poisons a fetched output again)
        pf, qf, x, r = G.to_field(g, pn_ref), G.to_field(g, q_ref), G.to_field(g, xc), G.to_field(g, rc)
        ss = _update(G, ws, g, alpha, pf, qf, x, r)
        x_ref, r_ref = xc + alpha * pn_ref, rc - alpha * q_ref
        assert np.array_equal(G.from_field(g, x), x_ref) and np.array_equal(G.from_field(g, r), r_ref)
        assert _close(ss, math.fsum(r_ref * r_ref)), (ss, math.fsum(r_ref * r_ref))
        if not big:
            x2, r2 = G.to_field(g, xc), G.to_field(g, rc)
            assert _update(G, ws, g, alpha, pf, qf, x2, r2) == ss
            assert np.array_equal(G.from_field(g, x2), x_ref) and np.array_equal(G.from_field(g, r2), r_ref)
            assert np.array_equal(G.from_field(g, pf), pn_ref) and np.array_equal(G.from_field(g, qf), q_ref)
            G.free(x2); G.free(r2)
        for f in (pf, qf, x, r):
            G.free(f)
        G.assert_no_leaks()
        assert G.guard_checks >= 8 and G.frame_checks >= 4
    finally:
        L.mgk_set_tuning(-1, -1)
        G.release()


def test_refusals(mgk, ws):
    """aliasing, a null argument, a hand-made geometry of even width, a call while the stream is being captured: MGK_EINVAL and no launch"""
    G = Guarded(mgk, poison=True)
    L = G.L
    g = G.geom(2, 15)
    z, p, pn, q = (G.to_field(g, np.ones(225)) for _ in range(4))
    x, r = G.to_field(g, np.ones(225)), G.to_field(g, np.ones(225))
    cf, s = G.coef(COEF2), C.c_double()
    EINVAL = 10001
    try:
        ws.poison()
        d = lambda gg, z_, po_, pn_, q_, w_: L.mgk_cg_direction_apply_dot_f64(G.ctx, C.byref(gg), cf, 0.5, z_, po_, pn_, q_, w_, C.byref(s), None)
        u = lambda gg, p_, q_, x_, r_, w_: L.mgk_cg_update_sumsq_f64(G.ctx, C.byref(gg), 0.5, p_, q_, x_, r_, w_, C.byref(s), None)
        for args in ((g, z, p, p, q, ws.p), (g, z, p, z, q, ws.p), (g, z, p, pn, z, ws.p), (g, z, p, pn, p, ws.p), (g, z, p, pn, pn, ws.p),
                     (g, None, p, pn, q, ws.p), (g, z, p, None, q, ws.p), (g, z, p, pn, None, ws.p), (g, z, p, pn, q, None)):
            assert d(*args) == EINVAL and "mgk_cg_direction_apply_dot_f64" in G.last_error()
        for args in ((g, pn, q, x, x, ws.p), (g, pn, pn, x, r, ws.p), (g, pn, q, pn, r, ws.p), (g, None, q, x, r, ws.p), (g, pn, q, x, None, ws.p),
                     (g, pn, q, x, r, None)):
            assert u(*args) == EINVAL and "mgk_cg_update_sumsq_f64" in G.last_error()
        even = Geom()
        assert L.mgk_geom_init(C.byref(even), 2, 2, 2, 1) != 0
        C.memmove(C.byref(even), C.byref(g), C.sizeof(Geom))
        even.nx = 14
        assert d(even, z, p, pn, q, ws.p) == EINVAL and "odd nx" in G.last_error()
        assert u(even, pn, q, x, r, ws.p) == EINVAL and "odd nx" in G.last_error()
        with capturing(mgk):
            rc_d, msg_d = d(g, z, p, pn, q, ws.p), G.last_error()
            rc_u, msg_u = u(g, pn, q, x, r, ws.p), G.last_error()
        assert rc_d == EINVAL and "captured" in msg_d and rc_u == EINVAL and "captured" in msg_u
        # nothing ran: the slots still hold the fill, the fields what they held
        assert np.all(np.isnan(ws.slots()))
        for f in (z, p, pn, q, x, r):
            assert np.array_equal(G.from_field(g, f), np.ones(225))
        # and the calls are taken again afterwards
        assert d(g, z, p, pn, q, ws.p) == 0 and u(g, pn, q, x, r, ws.p) == 0
        for f in (z, p, pn, q, x, r):
            G.free(f)
    finally:
        G.release()
