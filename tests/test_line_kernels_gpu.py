"""The y-line Jacobi kernels (csrc/mgk_line.hip) against tests/line_reference.py: mgk_line_forward_f64 and mgk_line_backward_f64.

  outputs        np.array_equal on z and u' (the kernels follow the reference operation for operation, no FMA)
  fields         uniform(-1, 1); fields are laid out by hand (offset = org + i pitch + j), so that even widths can be run too:
                 mgk_geom_init knows only the odd widths of level grids, the kernels take any
  interior only  z and u' start from a sentinel pattern (ghost ring, padding and 256 doubles past the field): everything outside the
                 interior keeps it; with unew aliasing u the ghost ring of u is still zero afterwards
  forms          from a guess and from the zero guess (u = NULL), unew == u and unew != u
  widths         1, 2, 3; 61 .. 65 and 123 .. 125 (the forward tile stores 62 columns per wave), 127 .. 129 (the backward tile 64); 255, 1023
  rows           the unrolled period of 32 rows, its table chunks of 16 and the ring of D rows: sizes below, at and above 8, 16, 32, 48, 64
                 and 96 (n = 7, 9, 15 .. 17, 31 .. 33, 47 .. 49, 63 .. 65, 95 .. 97) with every built depth (8, 16, 32)
  tables         tests/row_tables._rt_tables (S != N: a swapped neighbour or a reversed march shows), tests/coef_cases.distinct_row_tables
                 (all five of a row distinct, W != E as well, mixed signs) and levels of meshes 1 and 2 from the oracle's assembled rows
  store policy   both forced forms (mgk_set_tuning(variant = 0 / 1)) and the choice by size"""
import ctypes as C

import numpy as np
import pytest

import line_reference as LR
from oracle import Oracle
from coef_cases import distinct_row_tables
from row_tables import _rt_tables

pytestmark = pytest.mark.gpu
SENT = 12345.678
SIZES = [1, 2, 3, 7, 9, 15, 16, 17, 23, 25, 31, 32, 33, 47, 48, 49, 61, 62, 63, 64, 65, 95, 96, 97, 123, 124, 125, 127, 128, 129, 255, 1023]
# (npts, level, mesh): stretched levels, n = 63, 63, 3, 255, 1023
MESH_LEVELS = [(65, 0, 1), (129, 1, 2), (17, 2, 1), (257, 0, 2), (1025, 0, 1)]


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


def _put(mgk, g, inner, fill=0.0):
    """a device field: `fill` everywhere (and on 256 doubles past the end), `inner` on the interior"""
    raw = np.full(g.total + 256, fill)
    if inner is not None:
        raw[_index(g)] = inner
    return mgk.upload(raw)


def _get(mgk, g, p, fill):
    """the interior; everything else must still hold `fill`"""
    raw = mgk.download(p, g.total + 256)
    idx = _index(g)
    inner = raw[idx].copy()
    raw[idx] = fill
    assert np.all(raw == fill), "a cell outside the interior was written"
    return inner


def _run(mgk, n, ct, seed, policy=-1, depth=-1):
    L = mgk.L
    g = _geom(mgk, n)
    rng = np.random.default_rng(seed)
    b, u = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    scale = 0.8
    l, gg, q = LR.tables(ct)
    dct, dl, dg, dq = mgk.upload(ct), mgk.upload(l), mgk.upload(gg), mgk.upload(q)
    db, du = _put(mgk, g, b), _put(mgk, g, u)
    G = C.byref(g)
    ptrs = [dct, dl, dg, dq, db, du]
    L.mgk_set_tuning(policy, depth)
    try:
        for guess in (True, False):
            uin, uref = (du, u) if guess else (None, None)
            zref = LR.forward(ct, l, gg, b, uref)
            dz = _put(mgk, g, None, SENT)
            mgk._chk(L.mgk_line_forward_f64(mgk.ctx, G, dct, dl, dg, db, uin, dz, None))
            mgk.sync()
            assert np.array_equal(_get(mgk, g, dz, SENT), zref), ("z", n, guess)
            # the backward pass reads only the interior of z: the sentinels around it must not matter
            oref = LR.backward(q, scale, zref, uref)
            do = _put(mgk, g, None, SENT)
            mgk._chk(L.mgk_line_backward_f64(mgk.ctx, G, dq, scale, dz, uin, do, None))
            mgk.sync()
            assert np.array_equal(_get(mgk, g, do, SENT), oref), ("unew", n, guess)
            mgk.free(do)
            if guess:
                # in place (the normal use): u' lands in u, whose ghost ring stays zero
                da = _put(mgk, g, u)
                ptrs.append(da)
                mgk._chk(L.mgk_line_backward_f64(mgk.ctx, G, dq, scale, dz, da, da, None))
                mgk.sync()
                assert np.array_equal(_get(mgk, g, da, 0.0), oref), ("in place", n)
            mgk.free(dz)
        assert np.array_equal(_get(mgk, g, db, 0.0), b) and np.array_equal(_get(mgk, g, du, 0.0), u)     # the inputs are untouched
    finally:
        L.mgk_set_tuning(-1, -1)
        for p in ptrs:
            mgk.free(p)


@pytest.mark.parametrize("n", SIZES)
def test_line_passes_on_random_row_tables(mgk, n):
    ct = _rt_tables(np.random.default_rng(1000 + n), n)[0]
    _run(mgk, n, ct, 7 * n + 1)


@pytest.mark.parametrize("n", [1, 3, 17, 63, 64, 125, 255])
def test_line_passes_on_non_symmetric_row_tables(mgk, n):
    """every coefficient of a row distinct: W != E (a swapped x neighbour shows), S != N, mixed signs; and the swap does show in the reference"""
    ct = distinct_row_tables(np.random.default_rng(4000 + n), n)[0]
    _run(mgk, n, ct, 11 * n + 2)
    if n >= 3:
        rng = np.random.default_rng(n)
        b, u = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
        l, g, q = LR.tables(ct)
        sw = ct[:, [0, 3, 2, 1, 4]]
        assert not np.array_equal(LR.forward(ct, l, g, b, u), LR.forward(sw, l, g, b, u))


@pytest.mark.parametrize("npts,level,mesh", MESH_LEVELS)
def test_line_passes_on_stretched_levels(mgk, orc, npts, level, mesh):
    ct = LR.level_table(orc, npts, level, mesh)
    _run(mgk, ct.shape[0], ct, npts + 10 * level + mesh)


@pytest.mark.parametrize("depth", [8, 16, 32])
@pytest.mark.parametrize("n", [7, 9, 15, 17, 31, 32, 33, 47, 49, 63, 65, 125])
def test_every_prefetch_depth(mgk, n, depth):
    ct = _rt_tables(np.random.default_rng(2000 + n), n)[0]
    _run(mgk, n, ct, 3 * n + depth, depth=depth)


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("n", [3, 63, 125, 255])
def test_both_store_policies(mgk, n, policy):
    ct = _rt_tables(np.random.default_rng(3000 + n), n)[0]
    _run(mgk, n, ct, 5 * n + policy, policy=policy)


def test_refusals(mgk):
    """2-D only; z aliasing an input of the forward pass, unew aliasing z, a guess without the operator's table"""
    L = mgk.L
    g, g3 = _geom(mgk, 7), mgk.geom(3, 7)
    t = mgk.upload(np.ones(35))
    f, f2, f3 = _put(mgk, g, None), _put(mgk, g, None), _put(mgk, g, None)
    G = C.byref(g)
    assert L.mgk_line_forward_f64(mgk.ctx, C.byref(g3), t, t, t, f, None, f2, None) != 0
    assert L.mgk_line_forward_f64(mgk.ctx, G, t, t, t, f, None, f, None) != 0
    assert L.mgk_line_forward_f64(mgk.ctx, G, t, t, t, f, f2, f2, None) != 0
    assert L.mgk_line_forward_f64(mgk.ctx, G, None, t, t, f, f2, f3, None) != 0
    assert L.mgk_line_backward_f64(mgk.ctx, G, t, 0.8, f, None, f, None) != 0
    with pytest.raises(Exception, match="mgk_line_backward_f64"):
        mgk._chk(L.mgk_line_backward_f64(mgk.ctx, C.byref(g3), t, 0.8, f, None, f2, None))
    for p in (t, f, f2, f3):
        mgk.free(p)
