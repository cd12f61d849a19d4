"""The x-line Jacobi kernels (csrc/mgk_xline.hip) against tests/xline_reference.py: mgk_xline_forward_f64 and mgk_xline_backward_f64.

  outputs        np.array_equal on z and u' (the kernels follow the reference operation for operation, no FMA)
  fields         uniform(-1, 1); fields are laid out by hand (offset = org + i pitch + j), so that even widths can be run too
  interior only  every field -- inputs included -- starts from a sentinel pattern on the ghost ring, the padding and 256 doubles past the
                 field: the outputs keep it everywhere outside the interior, and the results show that no input's ghost ring or padding was
                 read (the kernels take the ghost values as zero without loading them)
  forms          from a guess and from the zero guess (u = NULL), unew == u and unew != u
  rows           1, 2, 3; 61 .. 65 and 123 .. 125 (the forward tile stores 62 rows per wave), 127 .. 129 (the backward tile 64); 255, 1023
  columns        the tile of 16 columns and the ring of D tiles unrolled D-fold: sizes below, at and above 16, 32, 48, 64 and 96
                 (n = 15 .. 17, 31 .. 33, 47 .. 49, 63 .. 65, 95 .. 97) with every built depth (1, 2, 3)
  tables         tests/coef_cases.distinct_row_tables (random, diagonally dominant, all five of a row distinct and varying with the row:
                 W != E, S != N -- a swapped neighbour, a transposed index or a reversed march shows) with an n x n table g at an odd and
                 at a line-wide row stride; the level tables of meshes 0 / 1 / 2 from the oracle's assembled rows, mesh 0 in the stride-0 form
  store policy   both forced forms (mgk_set_tuning(variant = 0 / 1)) and the choice by size"""
import ctypes as C

import numpy as np
import pytest

import line_reference as LR
import xline_reference as XR
from oracle import Oracle
from coef_cases import distinct_row_tables

pytestmark = pytest.mark.gpu
SENT = 12345.678
SIZES = [1, 2, 3, 7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 61, 62, 63, 64, 65, 95, 96, 97, 123, 124, 125, 127, 128, 129, 255, 1023]
# (npts, level, mesh): n = 63 (uniform: stride 0), 63, 63, 3, 1, 255, 255 (uniform)
MESH_LEVELS = [(65, 0, 0), (65, 0, 1), (129, 1, 2), (17, 2, 1), (17, 3, 2), (257, 0, 2), (257, 0, 0)]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _geom(mgk, n):
    """the level geometry of an n x n grid; an even n borrows the padding of n + 1 (the column past the interior is then a ghost column)"""
    g = mgk.geom(2, n | 1, n)
    g.nx = n
    return g


def _index(g):
    return g.org + np.arange(g.ny)[:, None] * g.pitch + np.arange(g.nx)[None, :]


def _put(mgk, g, inner, fill=SENT):
    """a device field: `fill` everywhere (and on 256 doubles past the end), `inner` on the interior"""
    raw = np.full(g.total + 256, fill)
    if inner is not None:
        raw[_index(g)] = inner
    return mgk.upload(raw)


def _get(mgk, g, p, fill=SENT):
    """the interior; everything else must still hold `fill`"""
    raw = mgk.download(p, g.total + 256)
    idx = _index(g)
    inner = raw[idx].copy()
    raw[idx] = fill
    assert np.all(raw == fill), "a cell outside the interior was written"
    return inner


def _run(mgk, n, ct, seed, policy=-1, depth=-1, stride=None):
    """stride None: the n x n table at a stride of n rounded up to 16 doubles; 0: one row for all (ct's rows are then all the same)"""
    L = mgk.L
    g = _geom(mgk, n)
    rng = np.random.default_rng(seed)
    b, u = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    scale = 0.8
    gt = XR.table(ct)
    gs = (n + 15) // 16 * 16 if stride is None else stride
    if gs == 0:
        assert all(np.array_equal(ct[i], ct[0]) for i in range(n))
        gdev = np.concatenate([gt[0], np.full(5, SENT)])
    else:
        gdev = np.full((n, gs), SENT)
        gdev[:, :n] = gt
        gdev = np.concatenate([gdev.ravel(), np.full(5, SENT)])
    dct, dg = mgk.upload(ct), mgk.upload(gdev)
    db, du = _put(mgk, g, b), _put(mgk, g, u)
    G = C.byref(g)
    ptrs = [dct, dg, db, du]
    L.mgk_set_tuning(policy, depth)
    try:
        for guess in (True, False):
            uin, uref = (du, u) if guess else (None, None)
            zref = XR.forward(ct, gt, b, uref)
            dz = _put(mgk, g, None)
            mgk._chk(L.mgk_xline_forward_f64(mgk.ctx, G, dct, dg, gs, db, uin, dz, None))
            mgk.sync()
            assert np.array_equal(_get(mgk, g, dz), zref), ("z", n, guess)
            oref = XR.backward(ct, gt, scale, zref, uref)
            do = _put(mgk, g, None)
            mgk._chk(L.mgk_xline_backward_f64(mgk.ctx, G, dct, dg, gs, scale, dz, uin, do, None))
            mgk.sync()
            assert np.array_equal(_get(mgk, g, do), oref), ("unew", n, guess)
            mgk.free(do)
            if guess:
                # in place (the normal use): u' lands in u, whose surroundings stay as they were
                da = _put(mgk, g, u)
                ptrs.append(da)
                mgk._chk(L.mgk_xline_backward_f64(mgk.ctx, G, dct, dg, gs, scale, dz, da, da, None))
                mgk.sync()
                assert np.array_equal(_get(mgk, g, da), oref), ("in place", n)
            mgk.free(dz)
        assert np.array_equal(_get(mgk, g, db), b) and np.array_equal(_get(mgk, g, du), u)     # the inputs are untouched
    finally:
        L.mgk_set_tuning(-1, -1)
        for p in ptrs:
            mgk.free(p)


@pytest.mark.parametrize("n", SIZES)
def test_xline_passes_on_non_symmetric_row_tables(mgk, n):
    ct = distinct_row_tables(np.random.default_rng(1000 + n), n)[0]
    _run(mgk, n, ct, 7 * n + 1)


@pytest.mark.parametrize("n", [3, 17, 63, 125])
def test_a_swapped_neighbour_shows_and_any_row_stride_is_taken(mgk, n):
    """the swap of W and E, of S and N, and a reversed march change the reference on these tables; the kernels take a table at an odd stride"""
    ct = distinct_row_tables(np.random.default_rng(4000 + n), n)[0]
    _run(mgk, n, ct, 11 * n + 2, stride=n + 2)
    rng = np.random.default_rng(n)
    b, u = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    g = XR.table(ct)
    z = XR.forward(ct, g, b, u)
    for sw in (ct[:, [0, 3, 2, 1, 4]], ct[:, [4, 1, 2, 3, 0]]):
        assert not np.array_equal(z, XR.forward(sw, g, b, u))
    assert not np.array_equal(z, XR.forward(ct, g[:, ::-1], b, u))


@pytest.mark.parametrize("npts,level,mesh", MESH_LEVELS)
def test_xline_passes_on_level_tables(mgk, orc, npts, level, mesh):
    ct = LR.level_table(orc, npts, level, mesh)
    n = ct.shape[0]
    if mesh == 0:
        ct = np.tile(ct[min(1, n - 1)], (n, 1))         # the product's uniform table: the level's five constants in every row
    _run(mgk, n, ct, npts + 10 * level + mesh, stride=0 if mesh == 0 else None)


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("n", [7, 15, 17, 31, 33, 47, 49, 63, 65, 95, 97, 125])
def test_every_prefetch_depth(mgk, n, depth):
    ct = distinct_row_tables(np.random.default_rng(2000 + n), n)[0]
    _run(mgk, n, ct, 3 * n + depth, depth=depth)


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("n", [3, 63, 125, 255])
def test_both_store_policies(mgk, n, policy):
    ct = distinct_row_tables(np.random.default_rng(3000 + n), n)[0]
    _run(mgk, n, ct, 5 * n + policy, policy=policy)


def test_refusals(mgk):
    """2-D only; z aliasing an input of the forward pass, unew aliasing z, no tables, a row stride below the width"""
    L = mgk.L
    g, g3 = _geom(mgk, 7), mgk.geom(3, 7)
    t = mgk.upload(np.ones(64))
    f, f2, f3 = _put(mgk, g, None), _put(mgk, g, None), _put(mgk, g, None)
    G = C.byref(g)
    assert L.mgk_xline_forward_f64(mgk.ctx, C.byref(g3), t, t, 0, f, None, f2, None) != 0
    assert L.mgk_xline_forward_f64(mgk.ctx, G, t, t, 0, f, None, f, None) != 0
    assert L.mgk_xline_forward_f64(mgk.ctx, G, t, t, 0, f, f2, f2, None) != 0
    assert L.mgk_xline_forward_f64(mgk.ctx, G, None, t, 0, f, f2, f3, None) != 0
    assert L.mgk_xline_forward_f64(mgk.ctx, G, t, None, 0, f, f2, f3, None) != 0
    assert L.mgk_xline_forward_f64(mgk.ctx, G, t, t, 6, f, f2, f3, None) != 0
    assert L.mgk_xline_backward_f64(mgk.ctx, G, t, t, 0, 0.8, f, None, f, None) != 0
    assert L.mgk_xline_backward_f64(mgk.ctx, G, t, t, 3, 0.8, f, None, f2, None) != 0
    with pytest.raises(Exception, match="mgk_xline_backward_f64"):
        mgk._chk(L.mgk_xline_backward_f64(mgk.ctx, C.byref(g3), t, t, 0, 0.8, f, None, f2, None))
    for p in (t, f, f2, f3):
        mgk.free(p)
