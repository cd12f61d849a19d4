"""The exact-FMA form of the fp64 3-D constant-coefficient kernels (madd<true>, csrc/mgk_dev.hpp) against the generic
form and the CPU oracle.  Where all six off-diagonal coefficients are +-2^e, e >= 0, the launchers of k_jacobi3_3d, k_jacobi2r, k_pj2r3 and
k_rrrow take the form whose off-diagonal terms are fused multiply-adds; MGK_TUNE_NO_EXACT_FMA (65) forces the generic form in the same
build.  Every fine-level pass of the 3-D cycle is run both ways (the kernels that kept the generic form alone, DESIGN.md section 4 (xix),
included: the variant must change nothing there either): the default run is np.array_equal to the run under 65 and to the oracle (boxes
the oracle's operators do not take: to three sweeps of mgk_jacobi_f64, whose k_stencil is pinned to the oracle by tests/test_kernels_gpu.py).

Coefficients: all 2^20; anisotropic 4 / 16 / 64; one off-diagonal 3 * 2^10 (the launcher must fall to the generic form and still equal the
oracle); all 0.25 (generic by the e >= 0 rule).  Fields: half of the points uniform in (-1, 1), half with magnitudes log-uniform over
1e-300 .. 1e6, one in twenty an exact zero.

Shapes.  k_jacobi3_3d (mgk_jacobi3_f64, mgk_jacobi3_sumsq_f64): the tile edges -- 120 columns per wave, TY rows, first and last plane.  The
row kernels: the smallest full-row shape each launcher admits -- 127 x 127 x 9 (one wave per row: k_jacobi2r with a norm, k_rrrow),
511 x 511 x 5 (k_pj2r3 is built for rows of 512 / 1024), 1023 x 1023 x 3 (the plain k_jacobi2r is the default from rows of 1024 on).
Sums of squares to 1e-13 relative against the oracle (the summation order differs); between the two forms of one
kernel they are the same double."""
import ctypes as C

import numpy as np
import pytest

from oracle import Oracle

pytestmark = pytest.mark.gpu
NO_EXACT_FMA = 65
SCALE = 6.0 / 7.0
RED_RTOL = 1e-13

P20, P10 = float(2 ** 20), float(2 ** 10)
COEFS = {
    "pow2_20": [P20, P20, P20, -6.0 * P20, P20, P20, P20],
    "aniso_4_16_64": [4.0, 16.0, 64.0, -168.0, 64.0, 16.0, 4.0],
    "one_3x2_10": [P10, P10, P10, -8.0 * P10, 3.0 * P10, P10, P10],      # j+1 has two mantissa bits: generic form
    "quarter": [0.25, 0.25, 0.25, -1.5, 0.25, 0.25, 0.25],               # e < 0: generic form
}


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(autouse=True)
def _default_tuning(mgk):
    yield
    mgk.L.mgk_set_tuning(-1, -1)


def _field(rng, n):
    x = rng.uniform(-1.0, 1.0, n)
    wide = rng.random(n) < 0.5
    x[wide] = np.sign(x[wide]) * 10.0 ** rng.uniform(-300.0, 6.0, int(wide.sum()))
    x[rng.random(n) < 0.05] = 0.0
    return x


class Box:
    def __init__(self, mgk, nx, ny, nz, seed):
        self.mgk, self.own = mgk, []
        self.g = mgk.geom(3, nx, ny, nz)
        rng = np.random.default_rng(seed)
        self.u, self.b = _field(rng, nx * ny * nz), _field(rng, nx * ny * nz)
        self.du, self.db = self.keep(mgk.to_field(self.g, self.u)), self.keep(mgk.to_field(self.g, self.b))

    def keep(self, p):
        self.own.append(p)
        return p

    def out(self, g=None):
        g = g or self.g
        f = self.keep(self.mgk.field(g))
        self.mgk._chk(self.mgk.L.mgk_memset0(self.mgk.ctx, f, 8 * g.total, None))
        return f

    def close(self):
        for p in self.own:
            self.mgk.free(p)


def _clean(mgk, g, f):
    raw, inner = mgk.raw_field(g, f), mgk.from_field(g, f)
    return np.count_nonzero(raw) == np.count_nonzero(inner)


# ---- the three-stage pass and its norm form ----
# (mgk_geom_init takes odd nx only: 119 unknowns are the 60 column pairs = 120 columns of exactly one wave tile, 121 one pair more)
J3_SHAPES = [(1, 1, 1), (5, 3, 2), (119, 4, 3), (121, 5, 4), (255, 9, 5), (1023, 9, 9)]


@pytest.mark.parametrize("cname", list(COEFS))
@pytest.mark.parametrize("nx,ny,nz", J3_SHAPES)
def test_three_stage_pass_both_forms(mgk, orc, nx, ny, nz, cname):
    As = COEFS[cname]
    dinv = 1.0 / As[3]
    t = Box(mgk, nx, ny, nz, 65000 + nx + 7 * ny + 13 * nz)
    L, g, coef, ss = mgk.L, C.byref(t.g), mgk.coef(As), C.c_double()
    # reference: three single sweeps in the generic form, and the norm of the input's residual
    L.mgk_set_tuning(NO_EXACT_FMA, -1)
    d1, d2, d3 = t.out(), t.out(), t.out()
    mgk._chk(L.mgk_jacobi_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, t.du, d1, None))
    mgk._chk(L.mgk_jacobi_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, d1, d2, None))
    mgk._chk(L.mgk_jacobi_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, d2, d3, None))
    want = mgk.from_field(t.g, d3)
    mgk._chk(L.mgk_residual_sumsq_f64(mgk.ctx, g, coef, t.db, t.du, C.byref(ss), None))
    in_want = ss.value
    if nx == ny:                                                     # the oracle's operators take these
        J = lambda x: orc.jacobi(3, nx, As, SCALE, t.b, x, nz=nz)
        j1 = J(t.u)
        assert np.array_equal(want, J(J(j1)))
        r0 = orc.sumsq(orc.residual(3, nx, As, t.b, t.u, nz=nz))
        assert abs(in_want - r0) <= RED_RTOL * r0
    got = {}
    for var, zc in ((-1, -1), (NO_EXACT_FMA, -1), (-1, 1), (NO_EXACT_FMA, 5), (-1, 5)):
        L.mgk_set_tuning(var, zc)
        o = t.out()
        mgk._chk(L.mgk_jacobi3_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, t.du, o, None))
        assert np.array_equal(mgk.from_field(t.g, o), want), f"mgk_jacobi3_f64 variant={var} zc={zc}"
        assert _clean(mgk, t.g, o)
        o = t.out()
        mgk._chk(L.mgk_jacobi3_sumsq_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, t.du, o, C.byref(ss), None))
        assert np.array_equal(mgk.from_field(t.g, o), want), f"mgk_jacobi3_sumsq_f64 variant={var} zc={zc}"
        assert abs(ss.value - in_want) <= RED_RTOL * in_want, f"mgk_jacobi3_sumsq_f64 variant={var} zc={zc}: {ss.value} vs {in_want}"
        assert _clean(mgk, t.g, o)
        got[(var, zc)] = ss.value
    # the same partial sums in the same order: the two forms give the same norm to the last bit
    assert got[(-1, -1)] == got[(NO_EXACT_FMA, -1)] and got[(-1, 5)] == got[(NO_EXACT_FMA, 5)]
    L.mgk_set_tuning(-1, -1)
    assert np.array_equal(mgk.from_field(t.g, t.du), t.u) and np.array_equal(mgk.from_field(t.g, t.db), t.b)
    t.close()


# ---- the row kernels of the two-sweep cycle ----
class Thin(Box):
    """n x n x nz with its coarse grid, and the oracle's operators on it"""

    def __init__(self, mgk, orc, n, nz, As, seed):
        super().__init__(mgk, n, n, nz, seed)
        self.orc, self.n, self.nz, self.As = orc, n, nz, As
        self.nc, self.nzc = (n - 1) // 2, (nz - 1) // 2
        self.gc = mgk.geom(3, self.nc, self.nc, self.nzc)
        self.uc = _field(np.random.default_rng(seed + 1), self.nc * self.nc * self.nzc)
        self.duc = self.keep(mgk.to_field(self.gc, self.uc))

    def J(self, u, zero_guess=False):
        return self.orc.jacobi(3, self.n, self.As, SCALE, self.b, u, zero_guess=zero_guess, nz=self.nz)

    def res(self, u):
        return self.orc.residual(3, self.n, self.As, self.b, u, nz=self.nz)

    def R(self, r):
        return self.orc.restrict(3, self.n, r, nzf=self.nz, nzc=self.nzc)

    def P(self, uc, u):
        return self.orc.prolong_add(3, self.n, uc, u, nzf=self.nz, nzc=self.nzc)


@pytest.mark.parametrize("cname", list(COEFS))
@pytest.mark.parametrize("n,nz", [(127, 9), (511, 5), (1023, 3)])
def test_row_kernels_both_forms_equal_the_oracle(mgk, orc, n, nz, cname):
    As = COEFS[cname]
    dinv = 1.0 / As[3]
    t = Thin(mgk, orc, n, nz, As, 66000 + n + nz)
    L, g, gc, coef, ss = mgk.L, C.byref(t.g), C.byref(t.gc), mgk.coef(As), C.c_double()
    j1 = t.J(t.u)
    j2 = t.J(j1)
    r0, r1 = orc.sumsq(t.res(t.u)), orc.sumsq(t.res(j1))
    z3 = t.J(t.J(t.J(np.zeros_like(t.u), zero_guess=True)))
    pj1 = t.J(t.P(t.uc, t.u))
    pj2 = t.J(pj1)
    zj2 = t.J(t.J(t.P(t.uc, np.zeros_like(t.u))))
    bc = t.R(t.res(t.u))
    bc1 = t.R(t.res(j1))
    jz1 = orc.jacobi(3, t.nc, As, SCALE, bc1, np.zeros_like(bc1), zero_guess=True, nz=t.nzc)
    sums = {}

    def field(name, var, f, want, coarse=False):
        gg = t.gc if coarse else t.g
        assert np.array_equal(mgk.from_field(gg, f), want), f"{name} variant={var}"
        assert _clean(mgk, gg, f), f"{name} variant={var}: a ghost or padding cell was written"

    def norm(name, var, want):
        assert abs(ss.value - want) <= RED_RTOL * want, f"{name} variant={var}: {ss.value} vs {want}"
        sums[(name, var)] = ss.value

    for var in (-1, NO_EXACT_FMA):
        L.mgk_set_tuning(var, -1)
        o = t.out()
        mgk._chk(L.mgk_jacobi_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, t.du, o, None))                  # k_jrow from rows of 1024 on
        field("mgk_jacobi_f64", var, o, j1)
        o = t.out()
        mgk._chk(L.mgk_jacobi_sumsq_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, t.du, o, C.byref(ss), None))
        field("mgk_jacobi_sumsq_f64", var, o, j1)
        norm("mgk_jacobi_sumsq_f64", var, r0)
        o = t.out()
        mgk._chk(L.mgk_jacobi2_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, t.du, o, None))                 # k_jacobi2b / k_jacobi2r
        field("mgk_jacobi2_f64", var, o, j2)
        o = t.out()
        mgk._chk(L.mgk_jacobi2_sumsq_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, t.du, o, C.byref(ss), None))
        field("mgk_jacobi2_sumsq_f64", var, o, j2)
        norm("mgk_jacobi2_sumsq_f64", var, r0)
        o = t.out()
        mgk._chk(L.mgk_jacobi2_sumsq_mid_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, t.du, o, C.byref(ss), None))
        field("mgk_jacobi2_sumsq_mid_f64", var, o, j2)
        norm("mgk_jacobi2_sumsq_mid_f64", var, r1)
        if L.mgk_jacobi2_zero_ok_f64(g) == 1:
            o = t.out()
            mgk._chk(L.mgk_jacobi2_zero_f64(mgk.ctx, g, coef, dinv, SCALE, t.db, o, None))              # k_jacobi2<.., 3, true>
            field("mgk_jacobi2_zero_f64", var, o, z3)
        o = t.out()
        mgk._chk(L.mgk_prolong_jacobi_f64(mgk.ctx, g, gc, coef, dinv, SCALE, t.db, t.duc, t.du, o, None))      # k_pjrow
        field("mgk_prolong_jacobi_f64", var, o, pj1)
        if L.mgk_prolong_jacobi2_ok_f64(g, gc) == 1:                                                    # rows of 512 / 1024: k_pj2r3
            o = t.out()
            mgk._chk(L.mgk_prolong_jacobi2_f64(mgk.ctx, g, gc, coef, dinv, SCALE, t.db, t.duc, t.du, o, None))
            field("mgk_prolong_jacobi2_f64", var, o, pj2)
            o = t.out()
            mgk._chk(L.mgk_interp_jacobi2_f64(mgk.ctx, g, gc, coef, dinv, SCALE, t.db, t.duc, o, None))
            field("mgk_interp_jacobi2_f64", var, o, zj2)
        else:
            assert n == 127
        oc = t.out(t.gc)
        mgk._chk(L.mgk_residual_restrict_f64(mgk.ctx, g, gc, coef, t.db, t.du, oc, None))               # k_rrrow
        field("mgk_residual_restrict_f64", var, oc, bc, coarse=True)
        assert L.mgk_sweep_residual_restrict_ok_f64(g, gc) == 1
        o, oc, ou = t.out(), t.out(t.gc), t.out(t.gc)
        mgk._chk(L.mgk_sweep_residual_restrict_f64(mgk.ctx, g, gc, coef, dinv, SCALE, t.db, t.du, o, oc, ou, dinv, SCALE, None))      # k_srr / k_srr4b
        field("mgk_sweep_residual_restrict_f64: swept field", var, o, j1)
        field("mgk_sweep_residual_restrict_f64: coarse right-hand side", var, oc, bc1, coarse=True)
        field("mgk_sweep_residual_restrict_f64: coarse zero-guess sweep", var, ou, jz1, coarse=True)
    L.mgk_set_tuning(-1, -1)
    for (name, var), v in sums.items():                              # same partial sums, same order: the same norm to the last bit
        assert v == sums[(name, -1)], name
    assert np.array_equal(mgk.from_field(t.g, t.du), t.u) and np.array_equal(mgk.from_field(t.g, t.db), t.b)
    t.close()


def test_copying_prolongation_form_on_power_of_two_coefficients(mgk, orc):
    """k_pj2r (MGK_TUNE_PJ2_COPY, 46) keeps the generic form: on the same coefficients and fields it equals the oracle like k_pj2r3"""
    As = COEFS["pow2_20"]
    t = Thin(mgk, orc, 511, 5, As, 67000)
    L, g, gc = mgk.L, C.byref(t.g), C.byref(t.gc)
    pj2 = t.J(t.J(t.P(t.uc, t.u)))
    L.mgk_set_tuning(46, -1)
    o = t.out()
    mgk._chk(L.mgk_prolong_jacobi2_f64(mgk.ctx, g, gc, mgk.coef(As), 1.0 / As[3], SCALE, t.db, t.duc, t.du, o, None))
    assert np.array_equal(mgk.from_field(t.g, o), pj2)
    L.mgk_set_tuning(-1, -1)
    t.close()
