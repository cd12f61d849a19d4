"""BASELINE config 5 -- mixed precision: fp32 smoother sweeps inside an fp64 defect-correction loop.
No reference counterpart exists; the arithmetic is defined by oracle/mgo_f32.c (same canonical order,
IEEE binary32, no FMA) and the HIP kernels (T = float, 4 unknowns per lane) must match it BIT FOR BIT;
acceptance of the scheme itself: it converges to the same fp64 stopping criterion and the same
known-answer error as the fp64 cycle."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("n", [1, 3, 7, 31, 63, 127, 255])
def test_fp32_kernels_bit_exact(mgk, orc, n):
    rng = np.random.default_rng(n)
    N = n ** 3
    As = orc.level_stencil(3, n + 2, 0)[0]
    dinv = 1.0 / As[3]
    u, b = rng.uniform(-1, 1, N).astype(np.float32), rng.uniform(-1, 1, N).astype(np.float32)
    g = mgk.geom32(n)
    du, db, dout = mgk.to_field32(g, u), mgk.to_field32(g, b), mgk.field32(g)
    coef = mgk.coef(As)
    L = mgk.L
    variants = [-1] if n < 255 else [-1, 0, 1, 2, 3]
    for v in variants:
        for zc in (-1, 5):
            L.mgk_set_tuning(v, zc)
            mgk._chk(L.mgk_jacobi_f32(mgk.ctx, C.byref(g), coef, dinv, 6.0 / 7.0, db, du, dout, None))
            assert np.array_equal(mgk.from_field32(g, dout), orc.jacobi32(n, As, 6.0 / 7.0, b, u))
            mgk._chk(L.mgk_residual_f32(mgk.ctx, C.byref(g), coef, db, du, dout, None))
            assert np.array_equal(mgk.from_field32(g, dout), orc.residual32(n, As, b, u))
    L.mgk_set_tuning(-1, -1)
    mgk._chk(L.mgk_jacobi_zero_f32(mgk.ctx, C.byref(g), dinv, 6.0 / 7.0, db, dout, None))
    assert np.array_equal(mgk.from_field32(g, dout), orc.jacobi32(n, As, 6.0 / 7.0, b, np.zeros(N, np.float32), zero_guess=True))
    if n >= 7:
        nc = (n - 1) // 2
        gc = mgk.geom32(nc)
        uc = rng.uniform(-1, 1, nc ** 3).astype(np.float32)
        duc, dbc = mgk.to_field32(gc, uc), mgk.field32(gc)
        mgk._chk(L.mgk_restrict_fw_f32(mgk.ctx, C.byref(g), C.byref(gc), du, dbc, None))
        assert np.array_equal(mgk.from_field32(gc, dbc), orc.restrict32(n, u))
        mgk._chk(L.mgk_prolong_add_f32(mgk.ctx, C.byref(g), C.byref(gc), duc, du, None))
        assert np.array_equal(mgk.from_field32(g, du), orc.prolong_add32(n, uc, u))
        mgk.free(duc); mgk.free(dbc)
    for p in (du, db, dout):
        mgk.free(p)


@pytest.mark.parametrize("n", [7, 63])
def test_bridges_fp64_fp32(mgk, orc, n):
    rng = np.random.default_rng(5 + n)
    N = n ** 3
    As = orc.level_stencil(3, n + 2, 0)[0]
    u, b = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    g, g32 = mgk.geom(3, n), mgk.geom32(n)
    du, db, dr32 = mgk.to_field(g, u), mgk.to_field(g, b), mgk.field32(g32)
    ss = C.c_double()
    mgk._chk(mgk.L.mgk_residual_f64_to_f32(mgk.ctx, C.byref(g), C.byref(g32), mgk.coef(As), db, du, dr32, C.byref(ss), None))
    r = orc.residual(3, n, As, b, u)
    assert np.array_equal(mgk.from_field32(g32, dr32), r.astype(np.float32))
    ref = orc.sumsq(r)
    assert abs(ss.value - ref) <= 1e-13 * ref
    e = rng.uniform(-1, 1, N).astype(np.float32)
    de = mgk.to_field32(g32, e)
    mgk._chk(mgk.L.mgk_correct_f64_from_f32(mgk.ctx, C.byref(g), C.byref(g32), de, du, None))
    assert np.array_equal(mgk.from_field(g, du), u + e.astype(np.float64))
    for p in (du, db, dr32, de):
        mgk.free(p)


@pytest.mark.parametrize("npts,levels", [(17, 3), (17, 4), (33, 4), (65, 6), (129, 7)])
def test_mixed_solve_matches_oracle_and_fp64_answer(orc, npts, levels):
    from multigrid_petsc_amd.solver import Solver
    scale = 6.0 / 7.0
    s = Solver(3, npts, levels, scale=scale, maxiter=60, precision="mixed")
    s.set_rhs_problem()
    it = s.solve()
    ref = orc.vcycle_mixed(npts, levels, maxiter=60, scale=scale)
    assert it == ref["iters"]
    assert np.max(np.abs(s.rnorm - ref["rnorm"]) / ref["rnorm"]) <= 1e-12
    assert np.array_equal(s.solution(), ref["u"])
    # the scheme: same stopping criterion in fp64, same known-answer error as the all-fp64 cycle
    assert s.rnorm[-1] <= 1e-7 * s.bnorm
    f = orc.vcycle(3, npts, levels, 3, 3, maxiter=60, scale=scale)
    assert abs(it - f["iters"]) <= 1
    h = 1.0 / (npts - 1)
    kat = 3 * math.pi ** 2 / ((12 / h ** 2) * math.sin(math.pi * h / 2) ** 2) - 1.0
    assert abs(s.error_norms()[0] - kat) <= 5e-7
    s.close()


@pytest.mark.parametrize("nf", [3, 7, 31, 127, 255])
def test_fused_residual_restrict_fp32_bit_exact(mgk, orc, nf):
    rng = np.random.default_rng(50 + nf)
    nc = (nf - 1) // 2
    As = orc.level_stencil(3, nf + 2, 0)[0]
    u, b = rng.uniform(-1, 1, nf ** 3).astype(np.float32), rng.uniform(-1, 1, nf ** 3).astype(np.float32)
    gf, gc = mgk.geom32(nf), mgk.geom32(nc)
    du, db, dbc = mgk.to_field32(gf, u), mgk.to_field32(gf, b), mgk.field32(gc)
    want = orc.restrict32(nf, orc.residual32(nf, As, b, u))
    for zc in (-1, 5):
        mgk.L.mgk_set_tuning(-1, zc)
        mgk._chk(mgk.L.mgk_memset0(mgk.ctx, dbc, 4 * gc.total, None))
        mgk._chk(mgk.L.mgk_residual_restrict_f32(mgk.ctx, C.byref(gf), C.byref(gc), mgk.coef(As), db, du, dbc, None))
        assert np.array_equal(mgk.from_field32(gc, dbc), want)
    mgk.L.mgk_set_tuning(-1, -1)
    for p in (du, db, dbc):
        mgk.free(p)


@pytest.mark.parametrize("n,variant", [(1, -1), (3, -1), (7, 0), (31, 2), (63, 1), (127, 6), (255, 9), (255, 3)])
def test_fused_correction_and_residual_bit_exact(mgk, orc, n, variant):
    """mgk_correct_residual_f64_f32 == mgk_correct_f64_from_f32 followed by mgk_residual_f64_to_f32"""
    rng = np.random.default_rng(900 + n)
    N = n ** 3
    As = orc.level_stencil(3, n + 2, 0)[0]
    u, b, e = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(-1, 1, N).astype(np.float32)
    g, g32 = mgk.geom(3, n), mgk.geom32(n)
    du, db, dun = mgk.to_field(g, u), mgk.to_field(g, b), mgk.field(g)
    de, dr32 = mgk.to_field32(g32, e), mgk.field32(g32)
    mgk._chk(mgk.L.mgk_memset0(mgk.ctx, dr32, 4 * g32.total, None))
    ss = C.c_double()
    ucorr = u + e.astype(np.float64)
    r = orc.residual(3, n, As, b, ucorr)
    for zc in (-1, 3):
        mgk.L.mgk_set_tuning(variant, zc)
        mgk._chk(mgk.L.mgk_correct_residual_f64_f32(mgk.ctx, C.byref(g), C.byref(g32), mgk.coef(As), db, du, de, dun, dr32, C.byref(ss), None))
        assert np.array_equal(mgk.from_field(g, dun), ucorr)
        assert np.array_equal(mgk.from_field32(g32, dr32), r.astype(np.float32))
        assert abs(ss.value - orc.sumsq(r)) <= 1e-13 * orc.sumsq(r)
        raw = mgk.raw_field(g, dun)                      # ghosts of the corrected field stay zero
        assert abs(np.abs(raw).sum() - np.abs(ucorr).sum()) <= 1e-9 * np.abs(ucorr).sum()
    mgk.L.mgk_set_tuning(-1, -1)
    for p in (du, db, dun, de, dr32):
        mgk.free(p)


def test_mixed_fused_outer_step_changes_nothing():
    from multigrid_petsc_amd.solver import Solver
    res = {}
    for fuse in (15, 31):
        s = Solver(3, 65, 6, scale=6.0 / 7.0, maxiter=60, precision="mixed", fuse=fuse)
        s.set_rhs_problem()
        it = s.solve()
        res[fuse] = (it, s.rnorm.copy(), s.solution())
        s.close()
    assert res[15][0] == res[31][0] and np.array_equal(res[15][2], res[31][2])
    assert np.abs(res[15][1] / res[31][1] - 1).max() <= 1e-13


@pytest.mark.parametrize("n", [1, 3, 7, 31, 63, 127, 255])
def test_two_fp32_sweeps_in_one_pass_bit_exact(mgk, orc, n):
    rng = np.random.default_rng(7000 + n)
    As = orc.level_stencil(3, n + 2, 0)[0]
    dinv = 1.0 / As[3]
    u, b = rng.uniform(-1, 1, n ** 3).astype(np.float32), rng.uniform(-1, 1, n ** 3).astype(np.float32)
    g = mgk.geom32(n)
    du, db, dout = mgk.to_field32(g, u), mgk.to_field32(g, b), mgk.field32(g)
    s = 6.0 / 7.0
    want = orc.jacobi32(n, As, s, b, orc.jacobi32(n, As, s, b, u))
    for var, zc in [(v, z) for v in (-1, 2) for z in (-1, 8, 13)]:
        mgk.L.mgk_set_tuning(var, zc)
        mgk._chk(mgk.L.mgk_memset0(mgk.ctx, dout, 4 * g.total, None))
        mgk._chk(mgk.L.mgk_jacobi2_f32(mgk.ctx, C.byref(g), mgk.coef(As), dinv, s, db, du, dout, None))
        assert np.array_equal(mgk.from_field32(g, dout), want)
    mgk.L.mgk_set_tuning(-1, -1)
    for p in (du, db, dout):
        mgk.free(p)


def test_mixed_cycle_with_fp32_two_sweep_passes_changes_nothing():
    """fuse bit 6 (+ a low pair_min_n) runs the fp32 legs' sweeps two per pass: same fields as one sweep per launch"""
    from multigrid_petsc_amd.solver import Solver
    res = {}
    for fuse, pmin in ((31, 0), (127, 7)):
        s = Solver(3, 65, 6, scale=6.0 / 7.0, maxiter=60, precision="mixed", fuse=fuse, pair_min_n=pmin)
        s.set_rhs_problem()
        it = s.solve()
        res[fuse] = (it, s.rnorm.copy(), s.solution())
        s.close()
    assert res[31][0] == res[127][0] and np.array_equal(res[31][2], res[127][2])
    assert np.abs(res[31][1] / res[127][1] - 1).max() <= 1e-13
