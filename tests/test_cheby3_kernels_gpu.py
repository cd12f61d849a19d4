"""KSPCHEBYSHEV with max_it = 3 in one pass (mgk_cheby3_2d_f64 / _sumsq / _zero, mgk_prolong_cheby3_2d_f64) and the Chebyshev form of the
LDS tail kernel (mgk_tail_cycle_cheby_f64) against the composition of the oracle's primitives on the same seeded inputs: a Jacobi sweep
with scale s = 2 / (emax + emin), then two recurrence steps (Oracle.cheby_step) -- fields bit for bit, sums of squares to 1e-13.
Reference operations: KSPSolve(KSPCHEBYSHEV) with max_it = v0 (src/solver.c:1531, :1536, :1542), which restarts the recurrence at
every call; MatMult(pro) + VecAXPY :1540-1541; VecNorm :1546."""
import ctypes as C

import numpy as np
import pytest

from cheby_reference import EIGS, cheb7, ksp_solve, ksp_solve_rt
from oracle import Oracle
from row_tables import _rt_apply, _rt_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# 1 .. 7: smaller than a wave tile; 119 / 121 / 239 / 241: one and two tiles of 60 column pairs, exactly and one pair over; 127 .. 1023 take
# the short-chunk form by default, 2047 / 4095 the marching one
SIZES_2D = [1, 3, 7, 63, 119, 121, 127, 239, 241, 255, 511, 1023, 2047, 4095]
# default choice; marching form (50), chunks of 4 (51) and 8 (52) rows forced; explicit chunk lengths; odd (58) / all (59) chunks marched downwards
VARIANTS = ((-1, -1), (50, -1), (51, -1), (52, -1), (-1, 1), (-1, 5), (-1, 64), (58, 12), (59, 5))


@pytest.mark.parametrize("n", SIZES_2D)
def test_cheby3_2d_bit_exact(mgk, orc, n):
    rng = np.random.default_rng(41000 + n)
    q = float((n + 1) ** 2)
    As = [q, q, -4.0 * q, q, q]
    dinv = 1.0 / As[2]
    N = n * n
    u, b = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    g = mgk.geom(2, n)
    du, db, dout = mgk.to_field(g, u), mgk.to_field(g, b), mgk.field(g)
    r0 = orc.residual(2, n, As, b, u)
    want_ss = orc.sumsq(r0)
    ss = C.c_double()
    L, coef = mgk.L, mgk.coef(As)
    for emin, emax in EIGS:
        c7 = cheb7(emin, emax)
        if (emin, emax) != EIGS[0]:
            assert c7[1] < 0.0 and c7[4] < 0.0                         # 1 - omega < 0 in both steps
        p3 = ksp_solve(orc, 2, n, As, b, u, 3, emin, emax, zero=False)
        z3 = ksp_solve(orc, 2, n, As, b, None, 3, emin, emax, zero=True)
        for var, zc in VARIANTS:
            tag = f"eig=({emin},{emax}) variant={var} zc={zc}"
            L.mgk_set_tuning(var, zc)
            mgk._chk(L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
            mgk._chk(L.mgk_cheby3_2d_f64(mgk.ctx, C.byref(g), coef, dinv, _dp(c7), None, None, db, du, dout, None))
            got = mgk.from_field(g, dout)
            assert np.array_equal(got, p3), f"{tag}: three steps, max diff {np.abs(got - p3).max()}"
            raw = mgk.raw_field(g, dout)
            assert abs(np.abs(raw).sum() - np.abs(got).sum()) <= 1e-9 * max(np.abs(got).sum(), 1e-300)      # ghosts / padding stay zero
            mgk._chk(L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
            mgk._chk(L.mgk_cheby3_2d_sumsq_f64(mgk.ctx, C.byref(g), coef, dinv, _dp(c7), None, None, db, du, dout, C.byref(ss), None))
            assert np.array_equal(mgk.from_field(g, dout), p3), f"{tag}: three steps + norm"
            assert abs(ss.value - want_ss) <= 1e-13 * want_ss, f"{tag}: norm {ss.value} vs {want_ss}"
            mgk._chk(L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
            mgk._chk(L.mgk_cheby3_2d_zero_f64(mgk.ctx, C.byref(g), coef, dinv, _dp(c7), None, None, db, dout, None))
            got = mgk.from_field(g, dout)
            assert np.array_equal(got, z3), f"{tag}: three steps from the zero guess, max diff {np.abs(got - z3).max()}"
    L.mgk_set_tuning(-1, -1)
    assert np.array_equal(mgk.from_field(g, du), u) and np.array_equal(mgk.from_field(g, db), b)
    c7 = cheb7(*EIGS[0])
    # in place on u is refused, as for the other multi-sweep passes; so is a call without the factors
    assert L.mgk_cheby3_2d_f64(mgk.ctx, C.byref(g), coef, dinv, _dp(c7), None, None, db, du, du, None) != 0
    assert L.mgk_cheby3_2d_f64(mgk.ctx, C.byref(g), coef, dinv, None, None, None, db, du, dout, None) != 0
    for p in (du, db, dout):
        mgk.free(p)


@pytest.mark.parametrize("nf", [3, 7, 63, 119, 127, 239, 255, 511, 1023, 2047, 4095])   # (nf = 2 nc + 1 with nc odd)
def test_prolongation_and_cheby3_2d_bit_exact(mgk, orc, nf):
    rng = np.random.default_rng(42000 + nf)
    nc = (nf - 1) // 2
    q = float((nf + 1) ** 2)
    As = [q, q, -4.0 * q, q, q]
    dinv = 1.0 / As[2]
    u, b, uc = rng.uniform(-1, 1, nf * nf), rng.uniform(-1, 1, nf * nf), rng.uniform(-1, 1, nc * nc)
    gf, gc = mgk.geom(2, nf), mgk.geom(2, nc)
    du, db, duc, dout = mgk.to_field(gf, u), mgk.to_field(gf, b), mgk.to_field(gc, uc), mgk.field(gf)
    x0 = orc.prolong_add(2, nf, uc, u)
    for emin, emax in EIGS:
        c7 = cheb7(emin, emax)
        x = ksp_solve(orc, 2, nf, As, b, x0, 3, emin, emax, zero=False)
        for var, zc in VARIANTS:
            mgk.L.mgk_set_tuning(var, zc)
            mgk._chk(mgk.L.mgk_memset0(mgk.ctx, dout, 8 * gf.total, None))
            mgk._chk(mgk.L.mgk_prolong_cheby3_2d_f64(mgk.ctx, C.byref(gf), C.byref(gc), mgk.coef(As), dinv, _dp(c7), None, None, db, duc, du, dout, None))
            got = mgk.from_field(gf, dout)
            assert np.array_equal(got, x), f"eig=({emin},{emax}) variant={var} zc={zc}: max diff {np.abs(got - x).max()}"
            raw = mgk.raw_field(gf, dout)
            assert abs(np.abs(raw).sum() - np.abs(got).sum()) <= 1e-9 * np.abs(got).sum()
    mgk.L.mgk_set_tuning(-1, -1)
    assert np.array_equal(mgk.from_field(gf, du), u) and np.array_equal(mgk.from_field(gc, duc), uc)
    for p in (du, db, duc, dout):
        mgk.free(p)


@pytest.mark.parametrize("n", [3, 7, 63, 127, 255, 511, 1023, 2047])
def test_cheby3_2d_on_row_tables(mgk, orc, n):
    """the same four entry points with per-row coefficient tables (stretched meshes): against the canonical term order in numpy"""
    rng = np.random.default_rng(43000 + n)
    ct, dt = _rt_tables(rng, n)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    g = mgk.geom(2, n)
    du, db, dout = mgk.to_field(g, u.ravel()), mgk.to_field(g, b.ravel()), mgk.field(g)
    dct, ddt = mgk.upload(ct.ravel()), mgk.upload(dt)
    rr = b - _rt_apply(ct, u)
    want_ss = float((rr * rr).sum())
    ss = C.c_double()
    L = mgk.L
    nc = (n - 1) // 2
    pro = n >= 3 and nc % 2 == 1                            # (a coarse grid exists: nc odd)
    if pro:
        uc = rng.uniform(-1, 1, nc * nc)
        gc = mgk.geom(2, nc)
        duc = mgk.to_field(gc, uc)
        x0 = orc.prolong_add(2, n, uc, u.ravel()).reshape(n, n)
    for emin, emax in EIGS:
        c7 = cheb7(emin, emax)
        p3 = ksp_solve_rt(ct, dt, b, u, 3, emin, emax, zero=False)
        z3 = ksp_solve_rt(ct, dt, b, None, 3, emin, emax, zero=True)
        for var, zc in ((-1, -1), (50, -1), (51, -1), (52, -1), (-1, 3), (-1, 16), (58, 16), (59, 16)):
            tag = f"eig=({emin},{emax}) variant={var} zc={zc}"
            L.mgk_set_tuning(var, zc)
            mgk._chk(L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
            mgk._chk(L.mgk_cheby3_2d_sumsq_f64(mgk.ctx, C.byref(g), None, 1.0, _dp(c7), dct, ddt, db, du, dout, C.byref(ss), None))
            assert np.array_equal(mgk.from_field(g, dout).reshape(n, n), p3), tag
            assert abs(ss.value - want_ss) <= 1e-12 * want_ss, tag
            mgk._chk(L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
            mgk._chk(L.mgk_cheby3_2d_f64(mgk.ctx, C.byref(g), None, 1.0, _dp(c7), dct, ddt, db, du, dout, None))
            assert np.array_equal(mgk.from_field(g, dout).reshape(n, n), p3), tag
            mgk._chk(L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
            mgk._chk(L.mgk_cheby3_2d_zero_f64(mgk.ctx, C.byref(g), None, 1.0, _dp(c7), dct, ddt, db, dout, None))
            assert np.array_equal(mgk.from_field(g, dout).reshape(n, n), z3), tag
            if pro:
                want = ksp_solve_rt(ct, dt, b, x0, 3, emin, emax, zero=False)
                mgk._chk(L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
                mgk._chk(L.mgk_prolong_cheby3_2d_f64(mgk.ctx, C.byref(g), C.byref(gc), None, 1.0, _dp(c7), dct, ddt, db, duc, du, dout, None))
                assert np.array_equal(mgk.from_field(g, dout).reshape(n, n), want), tag
    L.mgk_set_tuning(-1, -1)
    for p in [du, db, dout, dct, ddt] + ([duc] if pro else []):
        mgk.free(p)


def _tail_levels(n0, nlev):
    ns = [n0]
    for _ in range(nlev - 1):
        ns.append((ns[-1] - 1) // 2)
    return ns


V_TAIL = [(3, 3), (2, 1), (1, 4), (0, 0)]


@pytest.mark.parametrize("dim,n0,nlev", [(2, 63, 6), (2, 63, 3), (2, 31, 5), (2, 7, 3), (2, 7, 2), (3, 15, 4), (3, 15, 2), (3, 7, 3)])
@pytest.mark.parametrize("v", V_TAIL)
def test_cheby_tail_kernel_bit_exact(mgk, orc, dim, n0, nlev, v):
    """mgk_tail_cycle_cheby_f64 against the oracle's primitives walked over the tail levels: every KSPSolve the restarted recurrence
    (with 0 steps it still takes its first), residual + full weighting down, prolongation + v0 steps up"""
    rng = np.random.default_rng(44000 + 100 * dim + n0 + nlev)
    ns = _tail_levels(n0, nlev)
    v0, v1 = v

    def stencil(n):
        q = float((n + 1) ** 2)
        return [q, q, -4.0 * q, q, q] if dim == 2 else [q, q, q, -6.0 * q, q, q, q]
    Ass = [stencil(n) for n in ns]
    b0 = rng.uniform(-1, 1, n0 ** dim)
    g = mgk.geom(dim, n0)
    db, du = mgk.to_field(g, b0), mgk.field(g)
    nn = (C.c_int * nlev)(*ns)
    k7 = np.zeros(7 * nlev)
    di = np.zeros(nlev)
    for l, As in enumerate(Ass):
        k7[7 * l:7 * l + len(As)] = As
        di[l] = 1.0 / As[3 if dim == 3 else 2]
    for emin, emax in EIGS:
        B, U = [b0], []
        for l in range(nlev):
            U.append(ksp_solve(orc, dim, ns[l], Ass[l], B[l], None, v1 if l == nlev - 1 else v0, emin, emax, zero=True))
            if l < nlev - 1:
                B.append(orc.restrict(dim, ns[l], orc.residual(dim, ns[l], Ass[l], B[l], U[l])))
        for l in range(nlev - 2, -1, -1):
            U[l] = ksp_solve(orc, dim, ns[l], Ass[l], B[l], orc.prolong_add(dim, ns[l], U[l + 1], U[l]), v0, emin, emax, zero=False)
        mgk._chk(mgk.L.mgk_memset0(mgk.ctx, du, 8 * g.total, None))
        mgk._chk(mgk.L.mgk_tail_cycle_cheby_f64(mgk.ctx, C.byref(g), nlev, nn, _dp(k7), _dp(di), None, None, emin, emax, v0, v1, db, du, None))
        got = mgk.from_field(g, du)
        assert np.array_equal(got, U[0]), f"eig=({emin},{emax}): max diff {np.abs(got - U[0]).max()}"
    # more steps than the kernel's table, or eigenvalue bounds out of order: refused
    assert mgk.L.mgk_tail_cycle_cheby_f64(mgk.ctx, C.byref(g), nlev, nn, _dp(k7), _dp(di), None, None, 0.2, 2.0, 17, 3, db, du, None) != 0
    assert mgk.L.mgk_tail_cycle_cheby_f64(mgk.ctx, C.byref(g), nlev, nn, _dp(k7), _dp(di), None, None, 2.0, 0.2, 3, 3, db, du, None) != 0
    for p in (db, du):
        mgk.free(p)


@pytest.mark.parametrize("n0,nlev", [(63, 6), (31, 3), (7, 3)])
@pytest.mark.parametrize("v", V_TAIL)
def test_cheby_tail_kernel_on_row_tables(mgk, orc, n0, nlev, v):
    rng = np.random.default_rng(45000 + n0)
    ns = _tail_levels(n0, nlev)
    tabs = [_rt_tables(rng, n) for n in ns]
    b0 = rng.uniform(-1, 1, (n0, n0))
    v0, v1 = v
    g = mgk.geom(2, n0)
    db, du = mgk.to_field(g, b0.ravel()), mgk.field(g)
    dts = [(mgk.upload(ct.ravel()), mgk.upload(dt)) for ct, dt in tabs]
    cta = (C.c_void_p * nlev)(*[C.cast(a, C.c_void_p).value for a, _ in dts])
    dta = (C.c_void_p * nlev)(*[C.cast(d, C.c_void_p).value for _, d in dts])
    nn = (C.c_int * nlev)(*ns)
    for emin, emax in EIGS:
        B, U = [b0], []
        for l in range(nlev):
            U.append(ksp_solve_rt(*tabs[l], B[l], None, v1 if l == nlev - 1 else v0, emin, emax, zero=True))
            if l < nlev - 1:
                r = B[l] - _rt_apply(tabs[l][0], U[l])
                B.append(orc.restrict(2, ns[l], r.ravel()).reshape(ns[l + 1], ns[l + 1]))
        for l in range(nlev - 2, -1, -1):
            x = orc.prolong_add(2, ns[l], U[l + 1].ravel(), U[l].ravel()).reshape(ns[l], ns[l])
            U[l] = ksp_solve_rt(*tabs[l], B[l], x, v0, emin, emax, zero=False)
        mgk._chk(mgk.L.mgk_memset0(mgk.ctx, du, 8 * g.total, None))
        mgk._chk(mgk.L.mgk_tail_cycle_cheby_f64(mgk.ctx, C.byref(g), nlev, nn, None, None, cta, dta, emin, emax, v0, v1, db, du, None))
        got = mgk.from_field(g, du).reshape(n0, n0)
        assert np.array_equal(got, U[0]), f"eig=({emin},{emax}): max diff {np.abs(got - U[0]).max()}"
    for p in [db, du] + [x for t in dts for x in t]:
        mgk.free(p)
