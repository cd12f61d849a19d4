"""The three passes between the fp64 CG recurrence and the fp32 cycle (csrc/mgk_cg_mixed.hip, include/mgk_cg_mixed.h) on random fields, under
guarded.Guarded(mgk, poison=True): guard zones round every buffer, poisoned outputs, a zero frame.

  mgk_cg_dot_f64_f32                   sum r * (double) z32
  mgk_cg_direction_apply_dot_zf32_f64  p_new = (double) z32 + beta * p_old (first step: (double) z32), q = A p_new, sigma = p_new . q
  mgk_cg_update_sumsq_f64_f32          x += alpha * p, r -= alpha * q, sum r^2, r32 = (float) r, e0 = (float) scale * (r32 * (float) dinv)

  field outputs   np.array_equal to the numpy expressions in the stated order: z32.astype(float64) + beta * p_old, the canonical-order apply of
                  tests/test_cg_kernels_gpu.py, r.astype(float32), and the fp32 expression of e0 in numpy float32 arithmetic
  the three sums  within the bound of test_cg_kernels_gpu._close (1e-13 relative of math.fsum over the rounded products); the test asserts on its
                  own inputs that each sum is well conditioned (sum |terms| <= 4 |sum|): the coefficients have a dominant centre, and r of the dot
                  is z32 times a positive factor
  workspace       the partial slots are filled with NaN before EVERY call; twice: the same call again gives the same bits
  interior only   Guarded: nothing outside the interiors is written (the fp32 outputs included), the guards are intact, every output cell is written
  forms           p_old = NULL with the poisoned p_new lying about, e0 = NULL, both forced store policies, beta / alpha / dinv / scale no powers of two
  shapes          the 3-D shapes of tests/test_cg_kernels_gpu.py, a box of three different extents none a multiple of 16, one thin full-width box
  refusals        a 2-D geometry, aliases, null arguments, a capturing stream, more blocks than the workspace has slots"""
import ctypes as C
import math

import numpy as np
import pytest

from cg_kernel_aids import capturing
from guarded import Guarded
from multigrid_petsc_amd.mgk import Geom, cg_mixed_sigs
from test_cg_kernels_gpu import COEF3, SHAPES_3D, Ws, _apply, _close

pytestmark = pytest.mark.gpu
BOX = (37, 11, 23)
LARGE = (1023, 1023, 3)
CASES = [(s, -1) for s in SHAPES_3D + [BOX, LARGE]] + [((31, 31, 31), 0), ((31, 31, 31), 1), (BOX, 0), (BOX, 1)]
BETA, ALPHA, DINV, SCALE = 0.37, 0.61, 1.0 / 11.3, 0.8
EINVAL = 10001


def _id(c):
    return "x".join(str(n) for n in c[0]) + ("" if c[1] < 0 else f"-policy{c[1]}")


@pytest.fixture(scope="module")
def ws(mgk):
    cg_mixed_sigs(mgk.L)
    w = Ws(mgk)
    yield w
    w.close()


def _geoms(G, shape):
    g, g32 = G.geom(3, *shape), Geom()
    G._chk(G.L.mgk_geom_init_f32(C.byref(g32), 3, *shape))
    return g, g32


def _dot(G, ws, g, g32, r, z):
    ws.poison()
    s = C.c_double()
    G._chk(G.L.mgk_cg_dot_f64_f32(G.ctx, C.byref(g), C.byref(g32), r, z, ws.p, C.byref(s), None))
    return s.value


def _direction(G, ws, g, g32, beta, z, p_old, pn, q):
    ws.poison()
    s = C.c_double()
    G._chk(G.L.mgk_cg_direction_apply_dot_zf32_f64(G.ctx, C.byref(g), C.byref(g32), G.coef(COEF3), beta, z, p_old, pn, q, ws.p, C.byref(s), None))
    return s.value


def _update(G, ws, g, g32, p, q, x, r, r32, e0):
    ws.poison()
    s = C.c_double()
    G._chk(G.L.mgk_cg_update_sumsq_f64_f32(G.ctx, C.byref(g), C.byref(g32), ALPHA, p, q, x, r, r32, e0, DINV, SCALE, ws.p, C.byref(s), None))
    return s.value


def _conditioned(terms):
    exact = math.fsum(terms)
    assert math.fsum(np.abs(terms)) <= 4.0 * abs(exact)          # (a condition on the inputs)
    return exact


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_the_three_passes(mgk, ws, case):
    shape, policy = case
    G = Guarded(mgk, poison=True)
    L = G.L
    g, g32 = _geoms(G, shape)
    N = int(np.prod(shape))
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + shape[2])
    z32c = rng.uniform(-1, 1, N).astype(np.float32)
    zc = z32c.astype(np.float64)
    pc, xc, rc = (rng.uniform(-1, 1, N) for _ in range(3))
    L.mgk_set_tuning(policy, -1)
    try:
        big = N > 3000000                                   # the thin full-width box: one call of each pass (every fetch moves the whole field)
        z = G.to_field32(g32, z32c)
        # ---- the dot: r = z32 times a positive factor, so that the sum is well conditioned
        rdc = zc * rng.uniform(0.5, 1.5, N)
        rd = G.to_field(g, rdc)
        exact = _conditioned(rdc * zc)
        d = _dot(G, ws, g, g32, rd, z)
        nblk = int(np.sum(~np.isnan(ws.slots())))
        assert 1 <= nblk <= ws.n
        assert _close(d, exact), (d, exact)
        if not big:
            assert _dot(G, ws, g, g32, rd, z) == d
        G.free(rd)
        # ---- the direction pass
        p_old, pn, q = G.to_field(g, pc), G.field(g), G.field(g)
        if not big:
            # the first step: p_new = (double) z32; p_old is not given, and the poisoned p_new and q must not reach the sum
            sig = _direction(G, ws, g, g32, BETA, z, None, pn, q)
            q_ref = _apply(shape, COEF3, zc)
            assert np.array_equal(G.from_field(g, pn), zc) and np.array_equal(G.from_field(g, q), q_ref)
            assert _close(sig, _conditioned(zc * q_ref)), sig
        sig = _direction(G, ws, g, g32, BETA, z, p_old, pn, q)
        pn_ref = zc + BETA * pc
        q_ref = _apply(shape, COEF3, pn_ref)
        exact = _conditioned(pn_ref * q_ref)
        assert np.array_equal(G.from_field(g, pn), pn_ref) and np.array_equal(G.from_field(g, q), q_ref)
        assert _close(sig, exact), (sig, exact)
        if not big:
            assert _direction(G, ws, g, g32, BETA, z, p_old, pn, q) == sig
            assert np.array_equal(G.from_field(g, pn), pn_ref) and np.array_equal(G.from_field(g, q), q_ref)
            assert np.array_equal(G.from_field32(g32, z), z32c) and np.array_equal(G.from_field(g, p_old), pc)      # the inputs are as they were
        for f in (z, p_old, pn, q):
            G.free(f)
        # ---- the update, in place, with r32 and e0
        pf, qf, x, r = G.to_field(g, pn_ref), G.to_field(g, q_ref), G.to_field(g, xc), G.to_field(g, rc)
        r32, e0 = G.field32(g32), G.field32(g32)
        ss = _update(G, ws, g, g32, pf, qf, x, r, r32, e0)
        x_ref, r_ref = xc + ALPHA * pn_ref, rc - ALPHA * q_ref
        r32_ref = r_ref.astype(np.float32)
        e0_ref = np.float32(SCALE) * (r32_ref * np.float32(DINV))
        assert e0_ref.dtype == np.float32
        assert np.array_equal(G.from_field(g, x), x_ref) and np.array_equal(G.from_field(g, r), r_ref)
        assert np.array_equal(G.from_field32(g32, r32), r32_ref) and np.array_equal(G.from_field32(g32, e0), e0_ref)
        assert _close(ss, math.fsum(r_ref * r_ref)), (ss, math.fsum(r_ref * r_ref))
        if not big:
            # e0 = NULL: r32 alone; the same sum, the same bits
            x2, r2, r32b = G.to_field(g, xc), G.to_field(g, rc), G.field32(g32)
            assert _update(G, ws, g, g32, pf, qf, x2, r2, r32b, None) == ss
            assert np.array_equal(G.from_field(g, x2), x_ref) and np.array_equal(G.from_field(g, r2), r_ref)
            assert np.array_equal(G.from_field32(g32, r32b), r32_ref)
            assert np.array_equal(G.from_field(g, pf), pn_ref) and np.array_equal(G.from_field(g, qf), q_ref)
            for f in (x2, r2, r32b):
                G.free(f)
        for f in (pf, qf, x, r, r32, e0):
            G.free(f)
        G.assert_no_leaks()
        assert G.guard_checks >= 8 and G.frame_checks >= 6
    finally:
        L.mgk_set_tuning(-1, -1)
        G.release()


def test_refusals(mgk, ws):
    """a 2-D geometry, aliasing, a null argument, a call while the stream is being captured: MGK_EINVAL and no launch"""
    G = Guarded(mgk, poison=True)
    L = G.L
    g, g32 = _geoms(G, (15, 15, 15))
    N = 15 ** 3
    one = np.ones(N)
    z, r32, e0 = (G.to_field32(g32, one) for _ in range(3))
    p, pn, q, x, r = (G.to_field(g, one) for _ in range(5))
    cf, s = G.coef(COEF3), C.c_double()
    try:
        ws.poison()
        dot = lambda gg, hh, r_, z_, w_: L.mgk_cg_dot_f64_f32(G.ctx, C.byref(gg), C.byref(hh), r_, z_, w_, C.byref(s), None)
        d = lambda gg, hh, z_, po_, pn_, q_, w_: L.mgk_cg_direction_apply_dot_zf32_f64(G.ctx, C.byref(gg), C.byref(hh), cf, 0.5, z_, po_, pn_, q_, w_, C.byref(s), None)
        u = lambda gg, hh, p_, q_, x_, r_, r32_, e0_, w_: L.mgk_cg_update_sumsq_f64_f32(G.ctx, C.byref(gg), C.byref(hh), 0.5, p_, q_, x_, r_, r32_, e0_, DINV, SCALE, w_, C.byref(s), None)
        for args in ((g, g32, r, r, ws.p), (g, g32, None, z, ws.p), (g, g32, r, None, ws.p), (g, g32, r, z, None)):
            assert dot(*args) == EINVAL and "mgk_cg_dot_f64_f32" in G.last_error()
        for args in ((g, g32, z, p, p, q, ws.p), (g, g32, z, p, pn, p, ws.p), (g, g32, z, p, pn, pn, ws.p), (g, g32, z, p, z, q, ws.p), (g, g32, z, p, pn, z, ws.p),
                     (g, g32, z, z, pn, q, ws.p), (g, g32, None, p, pn, q, ws.p), (g, g32, z, p, None, q, ws.p), (g, g32, z, p, pn, None, ws.p), (g, g32, z, p, pn, q, None)):
            assert d(*args) == EINVAL and "mgk_cg_direction_apply_dot_zf32_f64" in G.last_error()
        for args in ((g, g32, pn, q, x, x, r32, e0, ws.p), (g, g32, pn, pn, x, r, r32, e0, ws.p), (g, g32, pn, q, pn, r, r32, e0, ws.p), (g, g32, pn, q, x, r, r32, r32, ws.p),
                     (g, g32, pn, q, x, r, x, e0, ws.p), (g, g32, pn, q, x, r, r32, r, ws.p), (g, g32, None, q, x, r, r32, e0, ws.p), (g, g32, pn, q, x, None, r32, e0, ws.p),
                     (g, g32, pn, q, x, r, None, e0, ws.p), (g, g32, pn, q, x, r, r32, e0, None)):
            assert u(*args) == EINVAL and "mgk_cg_update_sumsq_f64_f32" in G.last_error()
        # a 2-D geometry, a pair of geometries of different extents, an even width
        g2 = G.geom(2, 15)
        _, other32 = _geoms(G, (15, 15, 13))
        even = Geom()
        C.memmove(C.byref(even), C.byref(g), C.sizeof(Geom))
        even.nx = 14
        for gg, hh in ((g2, g32), (g, other32), (even, g32)):
            assert dot(gg, hh, r, z, ws.p) == EINVAL and "3-D level geometry" in G.last_error()
            assert d(gg, hh, z, p, pn, q, ws.p) == EINVAL and "3-D level geometry" in G.last_error()
            assert u(gg, hh, pn, q, x, r, r32, e0, ws.p) == EINVAL and "3-D level geometry" in G.last_error()
        with capturing(mgk):
            got = [(dot(g, g32, r, z, ws.p), G.last_error()), (d(g, g32, z, p, pn, q, ws.p), G.last_error()), (u(g, g32, pn, q, x, r, r32, e0, ws.p), G.last_error())]
        assert all(rc == EINVAL and "captured" in msg for rc, msg in got), got
        # nothing ran: the slots still hold the fill, the fields what they held
        assert np.all(np.isnan(ws.slots()))
        for f in (p, pn, q, x, r):
            assert np.array_equal(G.from_field(g, f), one)
        for f in (z, r32, e0):
            assert np.array_equal(G.from_field32(g32, f), one.astype(np.float32))
        # and the calls are taken again afterwards
        assert dot(g, g32, r, z, ws.p) == 0 and d(g, g32, z, p, pn, q, ws.p) == 0 and u(g, g32, pn, q, x, r, r32, e0, ws.p) == 0
        for f in (z, r32, e0, p, pn, q, x, r):
            G.free(f)
    finally:
        G.release()


@pytest.mark.parametrize("shape", [(1, 131073, 1), (1048577, 1, 1)], ids=["direction", "rows"])
def test_more_blocks_than_workspace_slots_is_refused(mgk, ws, shape):
    """shapes whose launch would need more blocks than the workspace has slots -- 32769 strips of the direction pass, 2049 blocks across a row
    of the two row walks: refused before anything is launched.  The buffers have the full size of the geometries all the same"""
    L = mgk.L
    err = Guarded(mgk, poison=False).last_error
    g, g32 = _geoms(mgk, shape)
    f64 = [mgk.alloc(8 * g.total) for _ in range(4)]
    f32 = [mgk.alloc(4 * g32.total) for _ in range(2)]
    s = C.c_double()
    try:
        ws.poison()
        p, pn, q, x = f64
        if shape[0] == 1:
            rc = L.mgk_cg_direction_apply_dot_zf32_f64(mgk.ctx, C.byref(g), C.byref(g32), mgk.coef(COEF3), 0.5, f32[0], p, pn, q, ws.p, C.byref(s), None)
            assert rc == EINVAL and "mgk_cg_direction_apply_dot_zf32_f64: more blocks than workspace slots" in err()
        else:
            rc = L.mgk_cg_dot_f64_f32(mgk.ctx, C.byref(g), C.byref(g32), p, f32[0], ws.p, C.byref(s), None)
            assert rc == EINVAL and "mgk_cg_dot_f64_f32: more blocks than workspace slots" in err()
            rc = L.mgk_cg_update_sumsq_f64_f32(mgk.ctx, C.byref(g), C.byref(g32), 0.5, p, pn, q, x, f32[0], f32[1], DINV, SCALE, ws.p, C.byref(s), None)
            assert rc == EINVAL and "mgk_cg_update_sumsq_f64_f32: more blocks than workspace slots" in err()
        assert np.all(np.isnan(ws.slots()))
    finally:
        for f in f64 + f32:
            mgk.free(f)
