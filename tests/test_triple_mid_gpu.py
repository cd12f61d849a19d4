"""The stacked three-sweep pass of the 3-D fine level (csrc/mgk_sweep3.hip k_jacobi3s, include/mgk_sweep3.h): eight waves of a block stacked
in y, two waves per SIMD, first / last rows of a wave exchanged through LDS.  Three forms: plain and with the norm of the input (the form the
three-sweep entry points take on these shapes; Tune.J3_3D_STACKED / _STACKED_DISPATCH name it, Tune.J3_3D_WAVES the older one), and mgk_jacobi3_sumsq_mid_f64, unew = J(J(J(u))) with
|| b - A J(u) ||^2.

Reference: three successive sweeps on seeded random u and b.  On cubes (ny = nx, thin in z) the sweeps are the CPU oracle's; on boxes, which
the oracle's 3-D operators do not take (they want nx = ny), they are tests/coef_cases.py np_sweep -- the oracle's arithmetic restated in numpy, held
to the oracle on the cubes here too.  Fields bit for bit (np.array_equal), sums of squares to 1e-13 (the figure of tests/test_kernels_gpu.py).

Shapes.  A block stores Y = 8 R - 6 rows: 26 (R = 4 rows per wave; plain and mid forms), 18 (R = 3; the form with the norm of the input).
ny in {1, 3, Y - 1, Y, Y + 1, 2 Y + 1, nx} for both Y; nz in {1, 2, 3, 4, 5, 9}: fewer planes than the pipeline is deep (4), that many, more;
chunk seams forced with zc in {1, 2, 5}; both tile orders.  nx in {511, 1023}: the two row widths the pass is built for (5 and 9 wave tiles
of 120 columns, the last one partly outside the grid)."""
import ctypes as C

import numpy as np
import pytest

from coef_cases import dense_field, distinct_coef, np_residual, np_sweep
from guarded import Guarded
from multigrid_petsc_amd import Tune
from multigrid_petsc_amd.mgk import MgkError
from oracle import Oracle

pytestmark = pytest.mark.gpu

SCALE = 0.8
RED_RTOL = 1e-13
WAVES, STACKED, DISPATCH, NO_EX = int(Tune.J3_3D_WAVES), int(Tune.J3_3D_STACKED), int(Tune.J3_3D_STACKED_DISPATCH), int(Tune.NO_EXACT_FMA)
Y4, Y3 = 26, 18
NYS = [1, 3, Y3 - 1, Y3, Y3 + 1, Y4 - 1, Y4, Y4 + 1, 2 * Y3 + 1, 2 * Y4 + 1]
NZS = [1, 2, 3, 4, 5, 9]
# every ny and every nz with both nx, not their product: nz walks through its list along the ny
BOXES = [(nx, ny, NZS[(i + k) % len(NZS)]) for k, nx in enumerate((511, 1023)) for i, ny in enumerate(NYS)]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _sumsq(orc, r):
    return orc.sumsq(np.ascontiguousarray(r).ravel())


def _reference(As, shape, seed):
    """(u, b, J(J(J(u))), b - A u, b - A J(u)) of seeded random fields, (nz, ny, nx) arrays, in the canonical arithmetic"""
    rng = np.random.default_rng(seed)
    u, b = dense_field(rng, *shape), dense_field(rng, *shape)
    j1 = np_sweep(As, SCALE, b, u)
    j3 = np_sweep(As, SCALE, b, np_sweep(As, SCALE, b, j1))
    return u, b, j3, np_residual(As, b, u), np_residual(As, b, j1)


def _run_forms(mgk, orc, g, As, ref, settings, mid_settings):
    """every form on the device fields of `ref`, under each (variant, zc) of `settings` (the three-sweep entry points: the variant names the
    stacked form) and of `mid_settings` (the mid form: always the stacked kernel)"""
    u, b, want, r0, r1 = ref
    L, coef, dinv = mgk.L, mgk.coef(list(As)), 1.0 / float(As[3])
    G = C.byref(g)
    du, db, out = mgk.to_field(g, u), mgk.to_field(g, b), mgk.field(g)
    want = want.ravel()
    in_want, mid_want = _sumsq(orc, r0), _sumsq(orc, r1)
    ss = C.c_double()

    def check(tag, norm=None):
        got = mgk.from_field(g, out)
        assert np.array_equal(got, want), f"{tag}: max diff {np.nanmax(np.abs(got - want))}, {np.count_nonzero(got != want)} cells differ"
        raw = mgk.raw_field(g, out)
        assert np.count_nonzero(raw) == np.count_nonzero(got), f"{tag}: the ghost ring or the padding of unew is not zero"
        if norm is not None:
            print(f"{tag}: sum {ss.value!r} reference {norm!r} rel {abs(ss.value - norm) / norm:.2e}")
            assert abs(ss.value - norm) <= RED_RTOL * norm, f"{tag}: {ss.value} vs {norm}"

    try:
        for var, zc in settings:
            L.mgk_set_tuning(var, zc)
            tag = f"{g.nx} x {g.ny} x {g.nz} variant={var} zc={zc}"
            mgk._chk(L.mgk_memset0(mgk.ctx, out, 8 * g.total, None))
            mgk._chk(L.mgk_jacobi3_f64(mgk.ctx, G, coef, dinv, SCALE, db, du, out, None))
            check("mgk_jacobi3_f64 " + tag)
            mgk._chk(L.mgk_memset0(mgk.ctx, out, 8 * g.total, None))
            ss.value = -1.0
            mgk._chk(L.mgk_jacobi3_sumsq_f64(mgk.ctx, G, coef, dinv, SCALE, db, du, out, C.byref(ss), None))
            check("mgk_jacobi3_sumsq_f64 " + tag, in_want)
        for var, zc in mid_settings:
            L.mgk_set_tuning(var, zc)
            tag = f"{g.nx} x {g.ny} x {g.nz} variant={var} zc={zc}"
            mgk._chk(L.mgk_memset0(mgk.ctx, out, 8 * g.total, None))
            ss.value = -1.0
            mgk._chk(L.mgk_jacobi3_sumsq_mid_f64(mgk.ctx, G, coef, dinv, SCALE, db, du, out, C.byref(ss), None))
            check("mgk_jacobi3_sumsq_mid_f64 " + tag, mid_want)
    finally:
        L.mgk_set_tuning(-1, -1)
    assert np.array_equal(mgk.from_field(g, du), u.ravel()) and np.array_equal(mgk.from_field(g, db), b.ravel()), "u or b was modified"
    for p in (du, db, out):
        mgk.free(p)


SEAMS = [(STACKED, -1), (STACKED, 1), (STACKED, 2), (STACKED, 5), (DISPATCH, -1), (DISPATCH, 2)]
MID_SEAMS = [(-1, -1), (-1, 1), (-1, 2), (-1, 5), (DISPATCH, -1), (DISPATCH, 5)]


@pytest.mark.parametrize("nx,ny,nz", BOXES)
def test_stacked_three_sweeps_on_boxes(mgk, orc, nx, ny, nz):
    """non-symmetric coefficients (the generic instance): every form == three sweeps bit for bit, the sums to 1e-13, u and b unchanged, the ghost
    ring and padding of unew zero; chunk seams every 1, 2, 5 planes; both tile orders"""
    As = distinct_coef(np.random.default_rng([41000, nx, ny, nz]), 3)
    assert mgk.L.mgk_jacobi3_mid_ok_f64(C.byref(mgk.geom(3, nx, ny, nz))) == 1
    _run_forms(mgk, orc, mgk.geom(3, nx, ny, nz), As, _reference(As, (nz, ny, nx), [41001, nx, ny, nz]), SEAMS, MID_SEAMS)


@pytest.mark.parametrize("nx,nz", [(511, 5), (1023, 3)])
def test_stacked_three_sweeps_on_thin_cubes_against_the_oracle(mgk, orc, nx, nz):
    """ny = nx: the reference is the CPU oracle's three sweeps and residuals (np_sweep is held to them on the way); the power-of-two
    stencil of a uniform level -- the exact-FMA instance, and the generic one under Tune.NO_EXACT_FMA (the mid form; the three-sweep
    entry points get it on the boxes of the next test)"""
    q = float((nx + 1) ** 2)
    As = np.array([q, q, q, -6.0 * q, q, q, q])
    ref = _reference(As, (nz, nx, nx), [42000, nx, nz])
    u, b, j3, r0, r1 = ref
    J = lambda x: orc.jacobi(3, nx, list(As), SCALE, b.ravel(), x, nz=nz)
    j1 = J(u.ravel())
    assert np.array_equal(J(J(j1)), j3.ravel()) and np.array_equal(orc.residual(3, nx, list(As), b.ravel(), j1, nz=nz), r1.ravel())
    assert np.array_equal(orc.residual(3, nx, list(As), b.ravel(), u.ravel(), nz=nz), r0.ravel())
    _run_forms(mgk, orc, mgk.geom(3, nx, nx, nz), As, ref, [(STACKED, -1), (DISPATCH, 2)], [(-1, -1), (NO_EX, -1), (NO_EX, 2), (-1, 1)])


@pytest.mark.parametrize("nx,ny,nz", [(511, 27, 9), (1023, 53, 5)])
def test_power_of_two_stencil_on_boxes(mgk, orc, nx, ny, nz):
    """the exact-FMA instance and, under Tune.NO_EXACT_FMA, the generic one on the same power-of-two stencil: the same doubles (on these
    shapes the three-sweep entry points take the stacked form by default, so NO_EXACT_FMA reaches its generic instance there too)"""
    q = float((nx + 1) ** 2)
    As = np.array([q, q, q, -6.0 * q, q, q, q])
    _run_forms(mgk, orc, mgk.geom(3, nx, ny, nz), As, _reference(As, (nz, ny, nx), [43000, nx, ny, nz]), SEAMS[:3] + [(-1, -1), (NO_EX, -1), (NO_EX, 2)], MID_SEAMS + [(NO_EX, -1), (NO_EX, 1)])


@pytest.mark.parametrize("nx,ny,nz", [(511, 53, 9), (1023, 27, 4), (1023, 19, 9)])
def test_old_and_new_form_agree(mgk, nx, ny, nz):
    """mgk_jacobi3_f64 / mgk_jacobi3_sumsq_f64: the independent-wave form (Tune.J3_3D_WAVES) and the stacked one write the same field and,
    to 1e-13, return the same sum"""
    rng = np.random.default_rng([44000, nx, ny, nz])
    As = distinct_coef(rng, 3)
    g = mgk.geom(3, nx, ny, nz)
    du, db = mgk.to_field(g, dense_field(rng, nz, ny, nx)), mgk.to_field(g, dense_field(rng, nz, ny, nx))
    L, coef, dinv, G = mgk.L, mgk.coef(list(As)), 1.0 / float(As[3]), C.byref(g)
    res = {}
    try:
        for var in (WAVES, STACKED, -1):
            L.mgk_set_tuning(var, -1)
            o1, o2, ss = mgk.field(g), mgk.field(g), C.c_double()
            mgk._chk(L.mgk_jacobi3_f64(mgk.ctx, G, coef, dinv, SCALE, db, du, o1, None))
            mgk._chk(L.mgk_jacobi3_sumsq_f64(mgk.ctx, G, coef, dinv, SCALE, db, du, o2, C.byref(ss), None))
            res[var] = (mgk.from_field(g, o1), mgk.from_field(g, o2), ss.value)
            mgk.free(o1), mgk.free(o2)
    finally:
        L.mgk_set_tuning(-1, -1)
    for var in (STACKED, -1):
        assert np.array_equal(res[var][0], res[WAVES][0]) and np.array_equal(res[var][1], res[WAVES][0])
        assert abs(res[var][2] - res[WAVES][2]) <= RED_RTOL * res[WAVES][2]
    mgk.free(du), mgk.free(db)


def test_refusals(mgk):
    """unew == u and unew == b are refused; so is every shape the stacked pass is not built for, with a message that says which it takes"""
    L = mgk.L
    As = [1.0, 1.0, 1.0, -6.0, 1.0, 1.0, 1.0]
    coef, ss = mgk.coef(As), C.c_double()
    g = mgk.geom(3, 511, 5, 3)
    f1, f2 = mgk.field(g), mgk.field(g)
    assert L.mgk_jacobi3_sumsq_mid_f64(mgk.ctx, C.byref(g), coef, -1 / 6.0, SCALE, f1, f2, f2, C.byref(ss), None) != 0      # unew == u
    assert L.mgk_jacobi3_sumsq_mid_f64(mgk.ctx, C.byref(g), coef, -1 / 6.0, SCALE, f1, f2, f1, C.byref(ss), None) != 0      # unew == b
    assert L.mgk_jacobi3_sumsq_mid_f64(mgk.ctx, C.byref(g), coef, -1 / 6.0, SCALE, f1, f2, None, C.byref(ss), None) != 0
    try:
        L.mgk_set_tuning(STACKED, -1)
        assert L.mgk_jacobi3_f64(mgk.ctx, C.byref(g), coef, -1 / 6.0, SCALE, f1, f2, f2, None) != 0
        assert L.mgk_jacobi3_sumsq_f64(mgk.ctx, C.byref(g), coef, -1 / 6.0, SCALE, f1, f2, f1, C.byref(ss), None) != 0
    finally:
        L.mgk_set_tuning(-1, -1)
    mgk.free(f1), mgk.free(f2)
    for dim, shape in ((3, (255, 255, 3)), (3, (127, 5, 5)), (3, (1021, 5, 5)), (3, (2047, 3, 3)), (3, (7, 511, 1023)), (2, (511, 511, 1))):
        g = mgk.geom(dim, *shape)
        assert L.mgk_jacobi3_mid_ok_f64(C.byref(g)) == 0
        f1, f2, f3 = mgk.field(g), mgk.field(g), mgk.field(g)
        with pytest.raises(MgkError, match="rows of 512 or 1024|3-D"):
            mgk._chk(L.mgk_jacobi3_sumsq_mid_f64(mgk.ctx, C.byref(g), coef, -1 / 6.0, SCALE, f1, f2, f3, C.byref(ss), None))
        if dim == 3:
            try:
                L.mgk_set_tuning(STACKED, -1)
                with pytest.raises(MgkError, match="rows of 512 or 1024"):
                    mgk._chk(L.mgk_jacobi3_f64(mgk.ctx, C.byref(g), coef, -1 / 6.0, SCALE, f1, f2, f3, None))
            finally:
                L.mgk_set_tuning(-1, -1)
        for p in (f1, f2, f3):
            mgk.free(p)
    assert L.mgk_jacobi3_mid_ok_f64(None) == 0


@pytest.mark.parametrize("form", ["plain", "norm", "mid"])
def test_forms_on_guarded_poisoned_buffers(mgk, orc, form):
    """one case per form between guard zones, the output's interior poisoned with NaN: nothing outside the allocation is written, the
    frame of unew holds zeros, no output cell is skipped or read"""
    gm = Guarded(mgk)
    nx, ny, nz = 511, 2 * Y4 + 1, 5
    As = distinct_coef(np.random.default_rng([45000, nx]), 3)
    name = {"plain": "mgk_jacobi3_f64", "norm": "mgk_jacobi3_sumsq_f64", "mid": "mgk_jacobi3_sumsq_mid_f64"}[form]
    gm.watch = frozenset([name])
    u, b, want, r0, r1 = _reference(As, (nz, ny, nx), [45001, nx])
    g = gm.geom(3, nx, ny, nz)
    L, coef, dinv, G = gm.L, gm.coef(list(As)), 1.0 / float(As[3]), C.byref(g)
    du, db, out, ss = gm.to_field(g, u), gm.to_field(g, b), gm.field(g), C.c_double()
    try:
        for var, zc in ((STACKED, -1), (DISPATCH, 2)):
            L.mgk_set_tuning(var, zc)
            if form == "plain":
                gm._chk(L.mgk_jacobi3_f64(gm.ctx, G, coef, dinv, SCALE, db, du, out, None))
            elif form == "norm":
                gm._chk(L.mgk_jacobi3_sumsq_f64(gm.ctx, G, coef, dinv, SCALE, db, du, out, C.byref(ss), None))
                assert abs(ss.value - _sumsq(orc, r0)) <= RED_RTOL * _sumsq(orc, r0)
            else:
                gm._chk(L.mgk_jacobi3_sumsq_mid_f64(gm.ctx, G, coef, dinv, SCALE, db, du, out, C.byref(ss), None))
                assert abs(ss.value - _sumsq(orc, r1)) <= RED_RTOL * _sumsq(orc, r1)
            assert np.array_equal(gm.from_field(g, out), want.ravel()), f"{name} variant={var} zc={zc}"
    finally:
        L.mgk_set_tuning(-1, -1)
    assert gm.poisoned_calls.get(name, 0) == 2, "the calls were not handed a poisoned output"
    assert np.array_equal(gm.from_field(g, du), u.ravel()) and np.array_equal(gm.from_field(g, db), b.ravel())
    for p in (du, db, out):
        gm.free(p)
    gm.assert_no_leaks()
