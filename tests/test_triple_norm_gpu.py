"""The input-norm form of the stacked three-sweep pass (csrc/mgk_sweep3.hip k_jacobi3s<R, 1>): what
mgk_jacobi3_sumsq_f64 takes on rows of 512 / 1024, unew = J(J(J(u))) and || b - A u ||^2 of the input.  Two forms inside one build: four rows
per wave (the default; a block stores Y = 26 rows) and, under TUNE_J3S_NORM_R3, three (Y = 18; the form before the accumulator pin).

Reference, on the same device fields under the default tuning: three mgk_jacobi_f64 (other tests hold that entry point to the oracle) for the
field, bit for bit; mgk_residual_f64 of the input for the norm: the float sum (math.fsum) of the squares of its interior, to RED_RTOL of
tests/test_exact_fma_gpu.py, the project's figure for these reductions.  Every case runs through the Guarded proxy: the output's interior is
poisoned with NaN and sits between guard zones, its ghost ring and padding must come back zero, the reduction scratch is poisoned before
every call, u and b must come back unchanged.

Shapes at the tile edges.  nx in {511, 1023}: the two row widths the pass is built for.  ny in {1, 25, 26, 27, 53}: Y - 1, Y, Y + 1 and
2 Y + 1 of the four-row form (53 is three blocks of the three-row form less one row).  nz in {1, 7, 8, 17}: fewer planes than the pipeline is
deep, one less than the shortest chunk the launcher cuts, that many, two chunks and one plane.  Every ny and every nz with both nx (nz walks
along the ny), each with both arithmetic instances: non-symmetric coefficients (the generic one) and the power-of-two stencil of a uniform
level (the exact-FMA one).  Chunk seams forced every 1, 2 and 5 planes through mgk_set_tuning's second argument, in both forms."""
import ctypes as C
import math

import numpy as np
import pytest

from coef_cases import dense_field, distinct_coef
from guarded import Guarded
from multigrid_petsc_amd import TUNE_J3S_NORM_R3
from test_exact_fma_gpu import RED_RTOL

pytestmark = pytest.mark.gpu

SCALE = 0.8
R3 = int(TUNE_J3S_NORM_R3)
NAME = "mgk_jacobi3_sumsq_f64"
NYS = [1, 25, 26, 27, 53]
NZS = [1, 7, 8, 17]
BOXES = [(nx, ny, NZS[(i + k) % len(NZS)]) for k, nx in enumerate((511, 1023)) for i, ny in enumerate(NYS)]
SETTINGS = [(var, zc) for var in (-1, R3) for zc in (-1, 1, 2, 5)]


def _coefficients(kind, nx, ny, nz):
    if kind == "pow2":
        q = float((nx + 1) ** 2)
        return np.array([q, q, q, -6.0 * q, q, q, q])
    return distinct_coef(np.random.default_rng([61000, nx, ny, nz]), 3)


@pytest.mark.parametrize("kind", ["generic", "pow2"])
@pytest.mark.parametrize("nx,ny,nz", BOXES)
def test_norm_and_three_sweeps(mgk, nx, ny, nz, kind):
    gm = Guarded(mgk)
    gm.watch = frozenset([NAME])
    As = _coefficients(kind, nx, ny, nz)
    rng = np.random.default_rng([61001, nx, ny, nz])
    g = gm.geom(3, nx, ny, nz)
    u, b = dense_field(rng, nz, ny, nx), dense_field(rng, nz, ny, nx)
    L, coef, dinv, G = gm.L, gm.coef(list(As)), 1.0 / float(As[3]), C.byref(g)
    du, db = gm.to_field(g, u), gm.to_field(g, b)
    t1, t2, t3, r, out = gm.field(g), gm.field(g), gm.field(g), gm.field(g), gm.field(g)
    gm._chk(L.mgk_jacobi_f64(gm.ctx, G, coef, dinv, SCALE, db, du, t1, None))
    gm._chk(L.mgk_jacobi_f64(gm.ctx, G, coef, dinv, SCALE, db, t1, t2, None))
    gm._chk(L.mgk_jacobi_f64(gm.ctx, G, coef, dinv, SCALE, db, t2, t3, None))
    gm._chk(L.mgk_residual_f64(gm.ctx, G, coef, db, du, r, None))
    want = gm.from_field(g, t3)
    res = gm.from_field(g, r)
    assert np.all(np.isfinite(want)) and np.count_nonzero(want) == want.size and np.all(np.isfinite(res))
    norm = math.fsum(res * res)
    assert norm > 0.0
    ss = C.c_double()
    try:
        for var, zc in SETTINGS:
            L.mgk_set_tuning(var, zc)
            tag = f"{nx} x {ny} x {nz} {kind} variant={var} zc={zc}"
            ss.value = -1.0
            gm._chk(L.mgk_jacobi3_sumsq_f64(gm.ctx, G, coef, dinv, SCALE, db, du, out, C.byref(ss), None))
            got = gm.from_field(g, out)                   # (asserts the guard zones and the zero frame of unew)
            assert np.array_equal(got, want), f"{tag}: max diff {np.nanmax(np.abs(got - want))}, {np.count_nonzero(got != want)} cells differ"
            print(f"{tag}: sum {ss.value!r} reference {norm!r} rel {abs(ss.value - norm) / norm:.2e}")
            assert abs(ss.value - norm) <= RED_RTOL * norm, f"{tag}: {ss.value!r} vs {norm!r}"
    finally:
        L.mgk_set_tuning(-1, -1)
    assert gm.poisoned_calls.get(NAME, 0) == len(SETTINGS), "the calls were not handed a poisoned output"
    assert gm.scratch_poisoned_calls.get(NAME, 0) == len(SETTINGS), "the reduction scratch was not poisoned before the calls"
    assert np.array_equal(gm.from_field(g, du), u.ravel()) and np.array_equal(gm.from_field(g, db), b.ravel()), "u or b was modified"
    for p in (du, db, t1, t2, t3, r, out):
        gm.free(p)
    gm.assert_no_leaks()


def test_the_two_forms_cut_different_blocks(mgk):
    """the switch reaches the launcher: on 1023 x 53 x 8 the four-row form reports 9 x 3 tiles of 26 rows, the three-row form 9 x 3 of 18 --
    the same count here, so the forms are told apart by their partial sums: the per-block partials differ, their totals agree to RED_RTOL"""
    gm = Guarded(mgk)
    nx, ny, nz = 1023, 53, 8
    As = _coefficients("generic", nx, ny, nz)
    rng = np.random.default_rng([61002])
    g = gm.geom(3, nx, ny, nz)
    L, coef, dinv, G = gm.L, gm.coef(list(As)), 1.0 / float(As[3]), C.byref(g)
    du, db, out = gm.to_field(g, dense_field(rng, nz, ny, nx)), gm.to_field(g, dense_field(rng, nz, ny, nx)), gm.field(g)
    parts, sums, ss = {}, {}, C.c_double()
    try:
        for var in (-1, R3):
            L.mgk_set_tuning(var, -1)
            gm._chk(L.mgk_jacobi3_sumsq_f64(gm.ctx, G, coef, dinv, SCALE, db, du, out, C.byref(ss), None))
            row = gm.read_scratch()
            parts[var], sums[var] = row[np.isfinite(row)], ss.value
    finally:
        L.mgk_set_tuning(-1, -1)
    assert abs(sums[-1] - sums[R3]) <= RED_RTOL * sums[-1], sums
    assert len(parts[-1]) > 1 and not np.array_equal(np.sort(parts[-1]), np.sort(parts[R3])), "both settings ran the same form"
    for p in (du, db, out):
        gm.free(p)
    gm.assert_no_leaks()
