"""The stacked three-sweep pass (csrc/mgk_sweep3.hip k_jacobi3s) on launches that take its XCD-contiguous tile order, under both load policies
of b: plain loads (the default) and the non-temporal ones it had before, TUNE_J3S_B_NT.  The other kernel tests
launch fewer than 64 blocks, where the tiles stay in dispatch order; two of the three boxes here do not:
    511 x 105 x 17, seams every 5 planes   5 x 5 tiles x 4 chunks = 100 tiles in 104 blocks: a padded launch (four dead blocks), more than one
                                            tile in every direction, the last tile in y clipped to one row
    1023 x 53 x 17, seams every 2 planes   9 x 3 tiles x 9 chunks = 243 tiles in 248 blocks
    511 x 209 x 8 (PRO: x 9), one chunk    5 x 9 = 45 tiles, below 64 blocks: the dispatch-order branch.  (The prolongation form needs an odd
                                            number of planes, 2 nzc + 1; 9 planes are still one chunk.)
The tile counts are the launcher's rule, ntx = ceil((nx + 1) / 2 / 60), nty = ceil(ny / 26), chunks of the forced length; the test asserts
them through the number of partial slots the norm forms write.

All four forms -- plain, norm of the input, norm of the first sweep's output (mid), prolongation form with a random coarse field -- with both
arithmetic instances (non-symmetric coefficients: the generic one; the power-of-two stencil: the exact-FMA one), each under the default and
under TUNE_J3S_B_NT, through the Guarded proxy: the output is poisoned and sits between guard zones, the reduction scratch is poisoned before
every reducing call, ghost ring and padding must come back zero and the inputs unchanged.
  field   bit for bit against three mgk_jacobi_f64 (PRO: mgk_prolong_jacobi_f64 and two mgk_jacobi_f64), computed once per box and instance
  sums    against math.fsum of the squares of mgk_residual_f64 (of u; mid: of J(u)) to RED_RTOL of tests/test_exact_fma_gpu.py
  and the sums under the two policies equal bit for bit: the policy changes no value, no partial slot and no order of the fixed-order sum."""
import ctypes as C
import math

import numpy as np
import pytest

from coef_cases import dense_field, distinct_coef
from guarded import Guarded, is_poison
from multigrid_petsc_amd import TUNE_J3S_B_NT
from test_exact_fma_gpu import RED_RTOL

pytestmark = pytest.mark.gpu

SCALE = 0.8
B_NT = int(TUNE_J3S_B_NT)
# (nx, ny, nz, forced chunk length, blocks the launch has)
BOXES = [(511, 105, 17, 5, 104), (1023, 53, 17, 2, 248), (511, 209, 8, -1, 45)]
PLAIN, NORM, MID, PRO = "mgk_jacobi3_f64", "mgk_jacobi3_sumsq_f64", "mgk_jacobi3_sumsq_mid_f64", "mgk_prolong_jacobi3_f64"


def _blocks(nx, ny, nz, zc):
    tiles = -(-((nx + 1) // 2) // 60) * -(-ny // 26) * (1 if zc <= 0 else -(-nz // zc))
    return tiles if tiles < 64 else (tiles + 7) & ~7


@pytest.mark.parametrize("kind", ["generic", "pow2"])
@pytest.mark.parametrize("nx,ny,nz,zc,nblk", BOXES)
def test_four_forms_under_both_policies(mgk, nx, ny, nz, zc, nblk, kind):
    assert _blocks(nx, ny, nz, zc) == nblk
    gm = Guarded(mgk)
    gm.watch = frozenset([PLAIN, NORM, MID, PRO])
    if kind == "pow2":
        q = float((nx + 1) ** 2)
        As = np.array([q, q, q, -6.0 * q, q, q, q])
    else:
        As = distinct_coef(np.random.default_rng([71000, nx, ny, nz]), 3)
    L, coef, dinv = gm.L, gm.coef(list(As)), 1.0 / float(As[3])
    rng = np.random.default_rng([71001, nx, ny, nz])
    ss = C.c_double()
    calls = {PLAIN: 0, NORM: 0, MID: 0, PRO: 0}
    # the prolongation form on an odd number of planes; the other three on the box as it stands
    for forms, nzf in (((PLAIN, NORM, MID), nz), ((PRO,), nz | 1)):
        g = gm.geom(3, nx, ny, nzf)
        gc = gm.geom(3, (nx - 1) // 2, (ny - 1) // 2, (nzf - 1) // 2)
        G, GC = C.byref(g), C.byref(gc)
        u, b = dense_field(rng, nzf, ny, nx), dense_field(rng, nzf, ny, nx)
        uc = dense_field(rng, gc.nz, gc.ny, gc.nx)
        du, db, duc = gm.to_field(g, u), gm.to_field(g, b), gm.to_field(gc, uc)
        t1, t2, t3, r, out = gm.field(g), gm.field(g), gm.field(g), gm.field(g), gm.field(g)
        # the references, once per field set, under the default tuning
        if forms == (PRO,):
            gm._chk(L.mgk_prolong_jacobi_f64(gm.ctx, G, GC, coef, dinv, SCALE, db, duc, du, t1, None))
        else:
            gm._chk(L.mgk_jacobi_f64(gm.ctx, G, coef, dinv, SCALE, db, du, t1, None))
        gm._chk(L.mgk_jacobi_f64(gm.ctx, G, coef, dinv, SCALE, db, t1, t2, None))
        gm._chk(L.mgk_jacobi_f64(gm.ctx, G, coef, dinv, SCALE, db, t2, t3, None))
        want = gm.from_field(g, t3)
        assert np.all(np.isfinite(want)) and np.count_nonzero(want) == want.size
        norms = {}
        for name, src in ((NORM, du), (MID, t1)):
            if name in forms:
                gm._chk(L.mgk_residual_f64(gm.ctx, G, coef, db, src, r, None))
                res = gm.from_field(g, r)
                norms[name] = math.fsum(res * res)
                assert np.all(np.isfinite(res)) and norms[name] > 0.0
        try:
            for name in forms:
                sums = {}
                for var in (-1, B_NT):
                    L.mgk_set_tuning(var, zc)
                    tag = f"{name} {nx} x {ny} x {nzf} {kind} variant={var} zc={zc}"
                    ss.value = -1.0
                    if name == PLAIN:
                        gm._chk(L.mgk_jacobi3_f64(gm.ctx, G, coef, dinv, SCALE, db, du, out, None))
                    elif name == PRO:
                        gm._chk(L.mgk_prolong_jacobi3_f64(gm.ctx, G, GC, coef, dinv, SCALE, db, duc, du, out, None))
                    else:
                        gm._chk(getattr(L, name)(gm.ctx, G, coef, dinv, SCALE, db, du, out, C.byref(ss), None))
                    calls[name] += 1
                    got = gm.from_field(g, out)               # (asserts the guard zones and the zero frame of unew)
                    assert np.array_equal(got, want), f"{tag}: max diff {np.nanmax(np.abs(got - want))}, {np.count_nonzero(got != want)} cells differ"
                    if name in norms:
                        wr = ~is_poison(gm.read_scratch())
                        assert wr[:nblk].all() and not wr[nblk:].any(), f"{tag}: {np.count_nonzero(wr)} partial slots written, {nblk} blocks"
                        print(f"{tag}: sum {ss.value!r} reference {norms[name]!r} rel {abs(ss.value - norms[name]) / norms[name]:.2e}")
                        assert abs(ss.value - norms[name]) <= RED_RTOL * norms[name], f"{tag}: {ss.value!r} vs {norms[name]!r}"
                        sums[var] = ss.value
                if name in norms:
                    assert sums[-1] == sums[B_NT], f"{name} {nx} x {ny} x {nzf} {kind}: the two policies sum differently: {sums}"
        finally:
            L.mgk_set_tuning(-1, -1)
        assert np.array_equal(gm.from_field(g, du), u.ravel()) and np.array_equal(gm.from_field(g, db), b.ravel()), "u or b was modified"
        assert np.array_equal(gm.from_field(gc, duc), uc.ravel()), "uc was modified"
        for p in (du, db, duc, t1, t2, t3, r, out):
            gm.free(p)
    for name, n in calls.items():
        assert n == 2 and gm.poisoned_calls.get(name, 0) == 2, f"{name}: the calls were not handed a poisoned output"
    for name in (NORM, MID):
        assert gm.scratch_poisoned_calls.get(name, 0) == 2, f"{name}: the reduction scratch was not poisoned before the calls"
    gm.assert_no_leaks()
