"""The prolongation form of the stacked three-sweep pass (csrc/mgk_sweep3.hip k_jacobi3s<.., PRO>, include/mgk_sweep3.h):
mgk_prolong_jacobi3_f64, unew = J(J(J(u + P uc))) in one pass -- the prolongation, its correction and three post-smoothing sweeps.

Reference: mgk_prolong_jacobi_f64 followed by two mgk_jacobi_f64 on the same device fields (other tests hold those entry points to the
oracle), under the default tuning; compared bit for bit (np.array_equal).  Every case runs through the Guarded proxy: the output's interior is
poisoned with NaN and sits between guard zones, its ghost ring and padding must come back zero, and u, b and uc must come back unchanged.

Shapes.  nx in {511, 1023}: the two row widths the pass is built for (5 and 9 wave tiles of 120 columns, the last one partly outside the
grid).  A block stores Y = 26 rows (R = 4 rows per wave); ny odd in {3, 17, 19, 25, 27, 37, 53}: Y +- 1 and 2 Y + 1 for Y = 26 and for the
three-row form's Y = 18.  nz odd in {3, 5, 9}, walked along the ny.  Chunk seams forced every 1, 2 and 5 planes: odd seams start a chunk on
an odd plane, where the parity that decides the parent planes is the global plane's, not the chunk's.  Both tile orders."""
import ctypes as C

import numpy as np
import pytest

from coef_cases import dense_field, distinct_coef
from guarded import Guarded
from multigrid_petsc_amd import Tune
from multigrid_petsc_amd.mgk import MgkError

pytestmark = pytest.mark.gpu

SCALE = 0.8
DISPATCH, NO_EX, NO_PRO = int(Tune.J3_3D_STACKED_DISPATCH), int(Tune.NO_EXACT_FMA), int(Tune.NO_PROLONG_TRIPLE)
NYS = [3, 17, 19, 25, 27, 37, 53]
NZS = [3, 5, 9]
# every ny and every nz with both nx, not their product: nz walks through its list along the ny
BOXES = [(nx, ny, NZS[(i + k) % len(NZS)]) for k, nx in enumerate((511, 1023)) for i, ny in enumerate(NYS)]
SEAMS = [(-1, -1), (-1, 1), (-1, 2), (-1, 5), (DISPATCH, -1), (DISPATCH, 2)]
NAME = "mgk_prolong_jacobi3_f64"


def _coarse(n):
    return (n - 1) // 2


def _run(mgk, shape, As, seed, settings):
    """the pass under each (variant, zc) of `settings` against prolongation + sweep, sweep, sweep on the same device fields"""
    nx, ny, nz = shape
    gm = Guarded(mgk)
    gm.watch = frozenset([NAME])
    rng = np.random.default_rng(seed)
    gf, gc = gm.geom(3, nx, ny, nz), gm.geom(3, _coarse(nx), _coarse(ny), _coarse(nz))
    u, b, uc = dense_field(rng, nz, ny, nx), dense_field(rng, nz, ny, nx), dense_field(rng, gc.nz, gc.ny, gc.nx)
    L, coef, dinv = gm.L, gm.coef(list(As)), 1.0 / float(As[3])
    GF, GC = C.byref(gf), C.byref(gc)
    du, db, duc = gm.to_field(gf, u), gm.to_field(gf, b), gm.to_field(gc, uc)
    t1, t2, t3, out = gm.field(gf), gm.field(gf), gm.field(gf), gm.field(gf)
    assert L.mgk_prolong_jacobi3_ok_f64(GF, GC) == 1
    gm._chk(L.mgk_prolong_jacobi_f64(gm.ctx, GF, GC, coef, dinv, SCALE, db, duc, du, t1, None))
    gm._chk(L.mgk_jacobi_f64(gm.ctx, GF, coef, dinv, SCALE, db, t1, t2, None))
    gm._chk(L.mgk_jacobi_f64(gm.ctx, GF, coef, dinv, SCALE, db, t2, t3, None))
    want = gm.from_field(gf, t3)
    assert np.all(np.isfinite(want)) and np.count_nonzero(want) == want.size
    try:
        for var, zc in settings:
            L.mgk_set_tuning(var, zc)
            tag = f"{nx} x {ny} x {nz} variant={var} zc={zc}"
            gm._chk(L.mgk_prolong_jacobi3_f64(gm.ctx, GF, GC, coef, dinv, SCALE, db, duc, du, out, None))
            got = gm.from_field(gf, out)                  # (asserts the guard zones and the zero frame of unew)
            assert np.array_equal(got, want), f"{tag}: max diff {np.nanmax(np.abs(got - want))}, {np.count_nonzero(got != want)} cells differ"
    finally:
        L.mgk_set_tuning(-1, -1)
    assert gm.poisoned_calls.get(NAME, 0) == len(settings), "the calls were not handed a poisoned output"
    assert np.array_equal(gm.from_field(gf, du), u.ravel()) and np.array_equal(gm.from_field(gf, db), b.ravel()), "u or b was modified"
    assert np.array_equal(gm.from_field(gc, duc), uc.ravel()), "uc was modified"
    for p in (du, db, duc, t1, t2, t3, out):
        gm.free(p)
    gm.assert_no_leaks()


@pytest.mark.parametrize("nx,ny,nz", BOXES)
def test_prolong_three_sweeps_on_boxes(mgk, nx, ny, nz):
    """non-symmetric coefficients (the generic instance): the pass == prolongation + sweep, sweep, sweep bit for bit; u, b and uc unchanged;
    ghost ring and padding of unew zero; chunk seams every 1, 2, 5 planes; both tile orders"""
    As = distinct_coef(np.random.default_rng([51000, nx, ny, nz]), 3)
    _run(mgk, (nx, ny, nz), As, [51001, nx, ny, nz], SEAMS)


@pytest.mark.parametrize("nx,nz", [(511, 5), (1023, 3)])
def test_power_of_two_stencil_on_thin_cubes(mgk, nx, nz):
    """ny = nx, the power-of-two stencil of a uniform level: the exact-FMA instance, and the generic one under Tune.NO_EXACT_FMA (the
    reference runs under the default tuning: the exact-FMA forms of its kernels)"""
    q = float((nx + 1) ** 2)
    As = np.array([q, q, q, -6.0 * q, q, q, q])
    _run(mgk, (nx, nx, nz), As, [52000, nx, nz], [(-1, -1), (-1, 1), (DISPATCH, 2), (NO_EX, -1), (NO_EX, 2)])


def test_refusals_and_the_switch(mgk):
    """wrong shapes, gf != 2 gc + 1 and unew aliasing an input are refused with MGK_EINVAL and a message; the _ok_ query says 0 for them and
    under Tune.NO_PROLONG_TRIPLE"""
    L = mgk.L
    coef = mgk.coef([1.0, 1.0, 1.0, -6.0, 1.0, 1.0, 1.0])
    gf, gc = mgk.geom(3, 511, 5, 3), mgk.geom(3, 255, 2, 1)
    assert L.mgk_prolong_jacobi3_ok_f64(C.byref(gf), C.byref(gc)) == 1
    try:
        L.mgk_set_tuning(NO_PRO, -1)
        assert L.mgk_prolong_jacobi3_ok_f64(C.byref(gf), C.byref(gc)) == 0
    finally:
        L.mgk_set_tuning(-1, -1)
    assert L.mgk_prolong_jacobi3_ok_f64(C.byref(gf), C.byref(gc)) == 1
    assert L.mgk_prolong_jacobi3_ok_f64(None, C.byref(gc)) == 0 and L.mgk_prolong_jacobi3_ok_f64(C.byref(gf), None) == 0
    u, b, o, uc = mgk.field(gf), mgk.field(gf), mgk.field(gf), mgk.field(gc)

    def call(gf_, gc_, b_, uc_, u_, o_):
        return L.mgk_prolong_jacobi3_f64(mgk.ctx, C.byref(gf_), C.byref(gc_), coef, -1 / 6.0, SCALE, b_, uc_, u_, o_, None)

    for args in ((b, uc, u, u), (b, uc, u, b), (b, uc, u, uc), (b, uc, u, None), (b, None, u, o)):      # unew == u, b, uc; missing fields
        with pytest.raises(MgkError, match="bad arguments"):
            mgk._chk(call(gf, gc, *args))
    for bad in (mgk.geom(3, 255, 3, 1), mgk.geom(3, 255, 2, 2), mgk.geom(3, 253, 2, 1), mgk.geom(2, 255, 2, 1)):      # gf != 2 gc + 1
        assert L.mgk_prolong_jacobi3_ok_f64(C.byref(gf), C.byref(bad)) == 0
        f = mgk.field(bad)
        with pytest.raises(MgkError, match="2 n \\+ 1"):
            mgk._chk(call(gf, bad, b, f, u, o))
        mgk.free(f)
    for p in (u, b, o, uc):
        mgk.free(p)
    for dim, fs, cs in ((3, (255, 255, 3), (127, 127, 1)), (3, (127, 5, 5), (63, 2, 2)), (3, (2047, 3, 3), (1023, 1, 1)), (3, (7, 511, 1023), (3, 255, 511)),
                        (2, (511, 511, 1), (255, 255, 1))):
        gf, gc = mgk.geom(dim, *fs), mgk.geom(dim, *cs)
        assert L.mgk_prolong_jacobi3_ok_f64(C.byref(gf), C.byref(gc)) == 0
        u, b, o, uc = mgk.field(gf), mgk.field(gf), mgk.field(gf), mgk.field(gc)
        with pytest.raises(MgkError, match="rows of 512 or 1024|3-D"):
            mgk._chk(call(gf, gc, b, uc, u, o))
        for p in (u, b, o, uc):
            mgk.free(p)
