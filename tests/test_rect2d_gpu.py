"""2-D grids with nx != ny.  include/mgk.h says "any vertex-centred 2-D grid" for the three-sweep, fused 2-D and row-table entry points and their
launchers accept rectangles, but every 2-D test of the core units (mgk_kernels.hip, mgk_sweep3.hip) is square: a row table indexed by the
column, an ny taken from nx, or a chunk count taken from the wrong axis is bit-identical there.

One body per shape, on guarded and poisoned buffers (tests/guarded.py), against tests/rect_reference.py (numpy; pinned to the oracle on squares
by tests/test_rect_reference_cpu.py).  Coefficients: distinct constants (tests/coef_cases.py, another set on the coarse level) and
distinct_row_tables (W != E, every row its own).  u, b, uc, then J, J^2, J^3, the residuals and norms, R(b - A .) and u + P uc are built once; every
2-D entry point that accepts the shape is compared: fields bit for bit, sums of squares to RED_RTOL of the reference sum.

Shapes (nx, ny): both orientations; nx and (nx - 1) / 2 odd, as mgk_geom_init needs; one and two wave tiles of the three-sweep kernels (120 columns
each), with the seam and without; each 2-D tile width of k_stencil; ny below, at and above a default chunk.  Tuning: the default, y chunks of 2 and
5, the forced forms 50 / 51 / 52 of the three-sweep passes, 55 / 56 of mgk_residual_restrict_2d_f64 and 38 of the 2-D mgk_prolong_jacobi_f64.

Every entry point compared here accepts these shapes (the ones that refuse rectangles, mgk_apply_add_f64, mgk_window_add_f64 and the tails, say so in
include/mgk.h and are not called): a refusal fails with the library's message."""
import ctypes as C

import numpy as np
import pytest

import rect_reference as RR
from cheby_reference import cheb7
from coef_cases import dense_field, distinct_coef, distinct_row_tables
from guarded import Guarded, MgkError
from oracle import Oracle

pytestmark = pytest.mark.gpu
RED_RTOL = 1e-13          # the project's figure for sums of squares (tests/test_kernels_gpu.py)
SUM_RTOL = 1e-12          # ... and for the error sums of mgk_error_sums_f64 (tests/test_kernels_gpu.py::test_rhs_fill_and_error_sums)
SC, SC_C = 6.0 / 7.0, 0.8
CHEB = (-0.37, 1.37, 0.21)
EIG = (0.5, 2.0)
SHAPES = [(119, 5), (7, 119), (243, 13), (15, 243), (63, 37), (39, 63), (511, 7)]          # (nx, ny)
BASE = ((-1, -1), (-1, 2), (-1, 5))
THREE = BASE + ((50, -1), (51, -1), (52, -1))
RR2D = BASE + ((55, -1), (56, -1))
PJ2D = BASE + ((38, -1),)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Rect:
    """one shape: the references, the device inputs, and the comparison of one call's outputs"""

    def __init__(self, G, orc, nx, ny):
        self.G, self.orc, self.L, self.nx, self.ny = G, orc, G.L, nx, ny
        rng = np.random.default_rng(95000 + 1000 * nx + ny)
        self.nyc, self.nxc = RR.coarse_shape(ny, nx)
        self.gf, self.gc = G.geom(2, nx, ny, 1), G.geom(2, self.nxc, self.nyc, 1)
        self.u, self.b, self.pm = (dense_field(rng, ny, nx) for _ in range(3))
        self.uc = dense_field(rng, self.nyc, self.nxc)
        self.As, self.Ac = distinct_coef(rng, 2, per_level=2)
        self.tab, self.tabc = distinct_row_tables(rng, ny), distinct_row_tables(rng, self.nyc)
        self.du, self.db, self.dpm, self.duc = G.to_field(self.gf, self.u), G.to_field(self.gf, self.b), G.to_field(self.gf, self.pm), G.to_field(self.gc, self.uc)
        self.dct, self.ddt, self.ddtc = G.upload(self.tab[0]), G.upload(self.tab[1]), G.upload(self.tabc[1])
        self.own = [self.du, self.db, self.dpm, self.duc, self.dct, self.ddt, self.ddtc]
        self.ss = C.c_double()

    def refs(self, ct, dt, dtc):
        """everything the calls are compared with, for one operator (fine tables ct / dt, coarse 1 / diag dtc), built once"""
        u, b, uc, pm = self.u, self.b, self.uc, self.pm
        J = lambda x: RR.sweep(ct, dt, SC, b, x)
        Jc0 = lambda bc: RR.sweep_zero(dtc, SC_C, bc)
        r = {}
        r["j1"] = J(u)
        r["j2"] = J(r["j1"])
        r["j3"] = J(r["j2"])
        r["z1"] = RR.sweep_zero(dt, SC, b)
        r["z3"] = J(J(r["z1"]))
        r["r0"] = RR.residual(ct, b, u)
        r["au"] = RR.apply(ct, u)
        r["ch"] = RR.cheby_step(ct, dt, b, u, pm, *CHEB)
        r["bc0"] = RR.restrict(r["r0"])
        r["bc1"] = RR.restrict(RR.residual(ct, b, r["j1"]))
        r["uc0_0"], r["uc0_1"] = Jc0(r["bc0"]), Jc0(r["bc1"])
        r["pu"] = RR.prolong_add(uc, u)
        r["pj1"] = J(r["pu"])
        r["pj3"] = J(J(r["pj1"]))
        r["i3"] = J(J(J(RR.prolong_add(uc, np.zeros_like(u)))))
        c7 = cheb7(*EIG)
        r["p3"], r["zc3"], r["pc3"] = RR.cheby3(ct, dt, c7, b, u), RR.cheby3(ct, dt, c7, b, None), RR.cheby3(ct, dt, c7, b, r["pu"])
        r["ss0"] = self.orc.sumsq(np.ascontiguousarray(r["r0"]).ravel())
        return r

    def out(self, coarse=False):
        return self.G.field(self.gc if coarse else self.gf)

    def call(self, name, tag, fn, outs, sumsq=None):
        """fn(): the return code.  outs: [(device field, is it coarse, reference)]; every output is freed here"""
        if sumsq is not None:
            self.ss.value = np.nan                   # a call that leaves its sum unwritten must not find the one before
        rc = fn()
        what = f"{name} {self.nx} x {self.ny} {tag}"
        try:
            try:
                self.G._chk(rc)
            except MgkError as e:
                raise AssertionError(f"{what}: {e}") from None
            for f, coarse, want in outs:
                got = self.G.from_field(self.gc if coarse else self.gf, f).reshape(want.shape)          # guards and frame
                bad = np.argwhere(got != want)
                assert bad.size == 0, f"{what}: {len(bad)} of {want.size} cells differ ({np.count_nonzero(np.isnan(got))} NaN), the first (i, j): {bad[:6].tolist()}"
            if sumsq is not None:
                assert abs(self.ss.value - sumsq) <= RED_RTOL * sumsq, f"{what}: sum of squares {self.ss.value!r} vs {sumsq!r}"
        finally:
            for f, _, _ in outs:
                self.G.free(f)

    def untouched(self):
        G = self.G
        assert np.array_equal(G.from_field(self.gf, self.du), self.u.ravel()) and np.array_equal(G.from_field(self.gf, self.db), self.b.ravel())
        assert np.array_equal(G.from_field(self.gf, self.dpm), self.pm.ravel()) and np.array_equal(G.from_field(self.gc, self.duc), self.uc.ravel())
        assert np.array_equal(G.download(self.dct, 5 * self.ny), self.tab[0].ravel()) and np.array_equal(G.download(self.ddt, self.ny), self.tab[1])

    def close(self):
        for p in self.own:
            self.G.free(p)


def _tune(L, var, zc):
    L.mgk_set_tuning(var, zc)
    return f"variant={var} zc={zc}"


def _constants(t):
    """every entry point on the constant stencil As (the coarse level's first sweep with ITS constants Ac)"""
    G, L, ctx, ss = t.G, t.L, t.G.ctx, C.byref(t.ss)
    g, gc, du, db, dpm, duc = C.byref(t.gf), C.byref(t.gc), t.du, t.db, t.dpm, t.duc
    As, coef = t.As, G.coef(t.As)
    dinv, dinv_c = 1.0 / As[2], 1.0 / t.Ac[2]
    ct, dt = RR.const_table(As, t.ny)
    r = t.refs(ct, dt, np.full(t.nyc, dinv_c))
    ny, c7k = t.ny, cheb7(*EIG)
    c7 = _dp(c7k)
    for var, zc in BASE:
        tag = _tune(L, var, zc)
        o = t.out()
        t.call("mgk_jacobi_f64", tag, lambda: L.mgk_jacobi_f64(ctx, g, coef, dinv, SC, db, du, o, None), [(o, 0, r["j1"])])
        o = t.out()

        def ranges():
            for z0, z1 in ((1, ny - 1), (0, 1), (ny - 1, ny)):
                rc = L.mgk_jacobi_range_f64(ctx, g, coef, dinv, SC, db, du, o, z0, z1, None)
                if rc:
                    return rc
            return 0
        t.call("mgk_jacobi_range_f64", tag, ranges, [(o, 0, r["j1"])])
        o = t.out()
        t.call("mgk_jacobi_zero_f64", tag, lambda: L.mgk_jacobi_zero_f64(ctx, g, dinv, SC, db, o, None), [(o, 0, r["z1"])])
        o = t.out()
        t.call("mgk_residual_f64", tag, lambda: L.mgk_residual_f64(ctx, g, coef, db, du, o, None), [(o, 0, r["r0"])])
        o = t.out()
        t.call("mgk_apply_f64", tag, lambda: L.mgk_apply_f64(ctx, g, coef, du, o, None), [(o, 0, r["au"])])
        o = t.out()
        t.call("mgk_cheby_f64", tag, lambda: L.mgk_cheby_f64(ctx, g, coef, dinv, *CHEB, db, du, dpm, o, None), [(o, 0, r["ch"])])
        t.call("mgk_sumsq_f64", tag, lambda: L.mgk_sumsq_f64(ctx, g, du, ss, None), [], t.orc.sumsq(t.u.ravel()))
        t.call("mgk_residual_sumsq_f64", tag, lambda: L.mgk_residual_sumsq_f64(ctx, g, coef, db, du, ss, None), [], r["ss0"])
        o = t.out()
        t.call("mgk_jacobi_sumsq_f64", tag, lambda: L.mgk_jacobi_sumsq_f64(ctx, g, coef, dinv, SC, db, du, o, ss, None), [(o, 0, r["j1"])], r["ss0"])
        o, o2 = t.out(), t.out()
        t.call("mgk_jacobi_sumsq_store_f64", tag, lambda: L.mgk_jacobi_sumsq_store_f64(ctx, g, coef, dinv, SC, None, None, db, du, o, o2, ss, None),
               [(o, 0, r["j1"]), (o2, 0, r["r0"])], r["ss0"])
        o = t.out()
        t.call("mgk_jacobi2_2d_f64", tag, lambda: L.mgk_jacobi2_2d_f64(ctx, g, coef, dinv, SC, db, du, o, None), [(o, 0, r["j2"])])
        o = t.out()
        t.call("mgk_jacobi2_2d_sumsq_f64", tag, lambda: L.mgk_jacobi2_2d_sumsq_f64(ctx, g, coef, dinv, SC, db, du, o, ss, None), [(o, 0, r["j2"])], r["ss0"])
        o = t.out(1)
        t.call("mgk_restrict_fw_f64", tag, lambda: L.mgk_restrict_fw_f64(ctx, g, gc, du, o, None), [(o, 1, RR.restrict(t.u))])
        o = G.to_field(t.gf, t.u)                               # in place: on a copy of u
        t.call("mgk_prolong_add_f64", tag, lambda: L.mgk_prolong_add_f64(ctx, g, gc, duc, o, None), [(o, 0, r["pu"])])
        o, o2, o3 = t.out(), t.out(1), t.out(1)
        t.call("mgk_sweep_residual_restrict_2d_f64", tag,
               lambda: L.mgk_sweep_residual_restrict_2d_f64(ctx, g, gc, coef, dinv, SC, db, du, o, o2, o3, dinv_c, SC_C, None),
               [(o, 0, r["j1"]), (o2, 1, r["bc1"]), (o3, 1, r["uc0_1"])])
        o, o2 = t.out(), t.out(1)
        t.call("mgk_sweep_residual_restrict_2d_f64", tag + " uc0=NULL",
               lambda: L.mgk_sweep_residual_restrict_2d_f64(ctx, g, gc, coef, dinv, SC, db, du, o, o2, None, dinv_c, SC_C, None),
               [(o, 0, r["j1"]), (o2, 1, r["bc1"])])
    for var, zc in RR2D:
        tag = _tune(L, var, zc)
        o, o2 = t.out(1), t.out(1)
        t.call("mgk_residual_restrict_2d_f64", tag, lambda: L.mgk_residual_restrict_2d_f64(ctx, g, gc, coef, db, du, o, o2, dinv_c, SC_C, None),
               [(o, 1, r["bc0"]), (o2, 1, r["uc0_0"])])
        o = t.out(1)
        t.call("mgk_residual_restrict_2d_f64", tag + " uc0=NULL", lambda: L.mgk_residual_restrict_2d_f64(ctx, g, gc, coef, db, du, o, None, dinv_c, SC_C, None),
               [(o, 1, r["bc0"])])
    for var, zc in PJ2D:
        tag = _tune(L, var, zc)
        o = t.out()
        t.call("mgk_prolong_jacobi_f64", tag, lambda: L.mgk_prolong_jacobi_f64(ctx, g, gc, coef, dinv, SC, db, duc, du, o, None), [(o, 0, r["pj1"])])
    for var, zc in THREE:
        tag = _tune(L, var, zc)
        _three(t, tag, r, coef, dinv, None, None, c7)
        o = t.out()
        t.call("mgk_interp_jacobi3_2d_f64", tag, lambda: L.mgk_interp_jacobi3_2d_f64(ctx, g, gc, coef, dinv, SC, db, duc, o, None), [(o, 0, r["i3"])])
    L.mgk_set_tuning(-1, -1)


def _three(t, tag, r, coef, dinv, dct, ddt, c7):
    """the three-sweep and Chebyshev three-step passes, constants (coef, dinv) or tables (dct, ddt; coef NULL, dinv ignored)"""
    G, L, ctx, ss = t.G, t.L, t.G.ctx, C.byref(t.ss)
    g, gc, du, db, duc = C.byref(t.gf), C.byref(t.gc), t.du, t.db, t.duc
    tag = tag + (" tables" if dct is not None else "")
    o = t.out()
    t.call("mgk_jacobi3_2d_f64", tag, lambda: L.mgk_jacobi3_2d_f64(ctx, g, coef, dinv, SC, dct, ddt, db, du, o, None), [(o, 0, r["j3"])])
    o = t.out()
    t.call("mgk_jacobi3_2d_sumsq_f64", tag, lambda: L.mgk_jacobi3_2d_sumsq_f64(ctx, g, coef, dinv, SC, dct, ddt, db, du, o, ss, None), [(o, 0, r["j3"])], r["ss0"])
    o, o2 = t.out(), t.out()
    t.call("mgk_jacobi3_2d_sumsq_store_f64", tag, lambda: L.mgk_jacobi3_2d_sumsq_store_f64(ctx, g, coef, dinv, SC, dct, ddt, db, du, o, o2, ss, None),
           [(o, 0, r["j3"]), (o2, 0, r["r0"])], r["ss0"])
    o = t.out()
    t.call("mgk_jacobi3_2d_zero_f64", tag, lambda: L.mgk_jacobi3_2d_zero_f64(ctx, g, coef, dinv, SC, dct, ddt, db, o, None), [(o, 0, r["z3"])])
    o = t.out()
    t.call("mgk_prolong_jacobi3_2d_f64", tag, lambda: L.mgk_prolong_jacobi3_2d_f64(ctx, g, gc, coef, dinv, SC, dct, ddt, db, duc, du, o, None), [(o, 0, r["pj3"])])
    o = t.out()
    t.call("mgk_cheby3_2d_f64", tag, lambda: L.mgk_cheby3_2d_f64(ctx, g, coef, dinv, c7, dct, ddt, db, du, o, None), [(o, 0, r["p3"])])
    o = t.out()
    t.call("mgk_cheby3_2d_sumsq_f64", tag, lambda: L.mgk_cheby3_2d_sumsq_f64(ctx, g, coef, dinv, c7, dct, ddt, db, du, o, ss, None), [(o, 0, r["p3"])], r["ss0"])
    o = t.out()
    t.call("mgk_cheby3_2d_zero_f64", tag, lambda: L.mgk_cheby3_2d_zero_f64(ctx, g, coef, dinv, c7, dct, ddt, db, o, None), [(o, 0, r["zc3"])])
    o = t.out()
    t.call("mgk_prolong_cheby3_2d_f64", tag, lambda: L.mgk_prolong_cheby3_2d_f64(ctx, g, gc, coef, dinv, c7, dct, ddt, db, duc, du, o, None), [(o, 0, r["pc3"])])


def _tables(t):
    """every row-table entry point on distinct_row_tables (the coarse level's first sweep with ITS 1 / diag table)"""
    G, L, ctx, ss = t.G, t.L, t.G.ctx, C.byref(t.ss)
    g, gc, du, db, dpm, duc, dct, ddt, ddtc = C.byref(t.gf), C.byref(t.gc), t.du, t.db, t.dpm, t.duc, t.dct, t.ddt, t.ddtc
    r = t.refs(t.tab[0], t.tab[1], t.tabc[1])
    c7k = cheb7(*EIG)
    c7 = _dp(c7k)
    for var, zc in BASE:
        tag = _tune(L, var, zc)
        for mode, want in ((0, r["j1"]), (1, r["r0"]), (4, r["au"])):
            o = t.out()
            t.call("mgk_rowcoef_f64", f"mode {mode} {tag}",
                   lambda: L.mgk_rowcoef_f64(ctx, g, mode, dct, ddt if mode == 0 else None, SC, None if mode == 4 else db, du, o, None), [(o, 0, want)])
        o = t.out()
        t.call("mgk_cheby_rowcoef_f64", tag, lambda: L.mgk_cheby_rowcoef_f64(ctx, g, dct, ddt, *CHEB, db, du, dpm, o, None), [(o, 0, r["ch"])])
        o = t.out()
        t.call("mgk_jacobi_zero_rowcoef_f64", tag, lambda: L.mgk_jacobi_zero_rowcoef_f64(ctx, g, ddt, SC, db, o, None), [(o, 0, r["z1"])])
        o = t.out()
        t.call("mgk_jacobi_sumsq_rowcoef_f64", tag, lambda: L.mgk_jacobi_sumsq_rowcoef_f64(ctx, g, dct, ddt, SC, db, du, o, ss, None), [(o, 0, r["j1"])], r["ss0"])
        t.call("mgk_residual_sumsq_rowcoef_f64", tag, lambda: L.mgk_residual_sumsq_rowcoef_f64(ctx, g, dct, db, du, ss, None), [], r["ss0"])
        o, o2 = t.out(), t.out()
        t.call("mgk_jacobi_sumsq_store_f64", tag + " tables", lambda: L.mgk_jacobi_sumsq_store_f64(ctx, g, None, 1.0, SC, dct, ddt, db, du, o, o2, ss, None),
               [(o, 0, r["j1"]), (o2, 0, r["r0"])], r["ss0"])
        o = t.out()
        t.call("mgk_jacobi2_2d_rowcoef_f64", tag, lambda: L.mgk_jacobi2_2d_rowcoef_f64(ctx, g, dct, ddt, SC, db, du, o, None), [(o, 0, r["j2"])])
        o = t.out()
        t.call("mgk_jacobi2_2d_sumsq_rowcoef_f64", tag, lambda: L.mgk_jacobi2_2d_sumsq_rowcoef_f64(ctx, g, dct, ddt, SC, db, du, o, ss, None), [(o, 0, r["j2"])], r["ss0"])
        o, o2 = t.out(1), t.out(1)
        t.call("mgk_residual_restrict_2d_rowcoef_f64", tag, lambda: L.mgk_residual_restrict_2d_rowcoef_f64(ctx, g, gc, dct, db, du, o, o2, ddtc, SC_C, None),
               [(o, 1, r["bc0"]), (o2, 1, r["uc0_0"])])
        o = t.out(1)
        t.call("mgk_residual_restrict_2d_rowcoef_f64", tag + " uc0=NULL", lambda: L.mgk_residual_restrict_2d_rowcoef_f64(ctx, g, gc, dct, db, du, o, None, None, SC_C, None),
               [(o, 1, r["bc0"])])
        o, o2, o3 = t.out(), t.out(1), t.out(1)
        t.call("mgk_sweep_residual_restrict_2d_rowcoef_f64", tag,
               lambda: L.mgk_sweep_residual_restrict_2d_rowcoef_f64(ctx, g, gc, dct, ddt, SC, db, du, o, o2, o3, ddtc, SC_C, None),
               [(o, 0, r["j1"]), (o2, 1, r["bc1"]), (o3, 1, r["uc0_1"])])
    for var, zc in PJ2D:
        tag = _tune(L, var, zc)
        o = t.out()
        t.call("mgk_prolong_jacobi_rowcoef_f64", tag, lambda: L.mgk_prolong_jacobi_rowcoef_f64(ctx, g, gc, dct, ddt, SC, db, duc, du, o, None), [(o, 0, r["pj1"])])
    for var, zc in THREE:
        _three(t, _tune(L, var, zc), r, None, 1.0, dct, ddt, c7)
    L.mgk_set_tuning(-1, -1)


def _setup_side(t):
    """mgk_fill_separable_f64 and mgk_error_sums_f64: the factors of x along the columns, of y along the rows"""
    G, L, ctx = t.G, t.L, t.G.ctx
    rng = np.random.default_rng(96000 + t.nx)
    cx, sy = dense_field(rng, t.nx), dense_field(rng, t.ny)
    dcx, dsy = G.upload(cx), G.upload(sy)
    o = t.out()
    t.call("mgk_fill_separable_f64", "", lambda: L.mgk_fill_separable_f64(ctx, C.byref(t.gf), dcx, dsy, dsy, o, None), [(o, 0, cx[None, :] * sy[:, None])])
    e3 = np.zeros(3)
    t.call("mgk_error_sums_f64", "", lambda: L.mgk_error_sums_f64(ctx, C.byref(t.gf), t.du, dcx, dsy, dsy, _dp(e3), None), [])
    e = np.abs(t.u - cx[None, :] * sy[:, None])
    assert e3[0] == e.max(), f"mgk_error_sums_f64: max {e3[0]!r} vs {e.max()!r}"
    assert abs(e3[1] - e.sum()) <= SUM_RTOL * e.sum() and abs(e3[2] - t.orc.sumsq(e.ravel())) <= RED_RTOL * t.orc.sumsq(e.ravel()), (e3, e.sum())
    G.free(dcx)
    G.free(dsy)


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_every_2d_entry_point_on_a_rectangle(mgk, orc, nx, ny):
    G = Guarded(mgk)
    try:
        t = Rect(G, orc, nx, ny)
        _constants(t)
        _tables(t)
        _setup_side(t)
        t.untouched()
        t.close()
        G.assert_no_leaks()
        assert G.frame_checks > 100
    finally:
        G.release()
        mgk.L.mgk_set_tuning(-1, -1)
