"""The Krylov orthogonalisation kernels (csrc/mgk_krylov.hip) on random fields: mgk_multi_dot_f64, mgk_multi_axpy_sumsq_f64 (+ mgk_krylov_fetch),
mgk_lincomb_f64, mgk_scale_to_f64.  A x on the row-table operator needs no new entry point: mgk_rowcoef_f64 (mode 4) gives it, and
tests/test_gmres_solve_gpu.py runs it inside the solves on the stretched meshes.

  field outputs   np.array_equal to the numpy expression in the stated order (ascending i, multiply and add / subtract rounded separately)
  dots, sumsq     within 1e-13 relative of math.fsum over the rounded products; the fields are mixed-sign but correlated, so that the dots are
                  well conditioned and "relative" means relative to the value itself
  interior only   every output starts from a sentinel pattern: cells outside the interior keep it, cells past the field too; and after
                  the multi-axpy, mgk_apply_f64 on the result equals the oracle's A x bit for bit (a written ghost cell would show there)
  shapes          2-D n = 1, 15, 63, 127 and 3-D 7^3, 31^3 with k = 1, 2, 7, 31 (every built width but 16 .. 33: k = 31 runs the widest);
                  1023^2, 4095^2 (k = 3: eight blocks per row, 134 MB per field) and the thin n x n x 3 with n = 511, 1023; n = 2 is not a
                  level geometry (mgk_geom_init refuses even widths) and the kernels refuse a hand-made one
  store policy    both forced forms (mgk_set_tuning(variant = 0 / 1)) and the choice by size"""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import Oracle

pytestmark = pytest.mark.gpu
SENT = 12345.678
KMAX = 33
SMALL = [(2, 1, 1), (2, 15, 1), (2, 63, 1), (2, 127, 1), (3, 7, 7), (3, 31, 31)]
LARGE = [(2, 1023, 1, 3), (2, 1023, 1, 7), (2, 4095, 1, 3), (3, 511, 3, 3), (3, 1023, 3, 3)]
SHAPES = [(d, n, nz, k, -1) for d, n, nz in SMALL for k in (1, 2, 7, 31)] + [(d, n, nz, k, -1) for d, n, nz, k in LARGE] + \
         [(2, 127, 1, 7, 0), (2, 127, 1, 7, 1), (3, 31, 31, 31, 0), (3, 31, 31, 31, 1), (2, 1023, 1, 3, 0), (2, 1023, 1, 3, 1)]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _ptrs(fields):
    return (C.c_void_p * len(fields))(*[f.value for f in fields])


def _geom(mgk, dim, n, nz):
    return mgk.geom(dim, n, n, nz if dim == 3 else 1)


class Sentinel:
    """a field whose every cell, ghosts included, and 256 doubles past its end hold a sentinel; optionally the interior holds `inner`"""

    def __init__(self, mgk, g, inner=None):
        self.mgk, self.g = mgk, g
        ones = mgk.to_field(g, np.ones(g.nx * g.ny * g.nz))
        self.mask = mgk.raw_field(g, ones) == 1.0
        mgk.free(ones)
        raw = np.full(g.total + 256, SENT)
        if inner is not None:
            raw[:g.total][self.mask] = np.asarray(inner).ravel()
        self.p = mgk.upload(raw)

    def interior(self):
        """the interior after a kernel ran; everything else must still be the sentinel"""
        raw = self.mgk.download(self.p, self.g.total + 256)
        assert np.all(raw[self.g.total:] == SENT), "a write past the field"
        assert np.all(raw[:self.g.total][~self.mask] == SENT), "a cell outside the interior was written"
        return raw[:self.g.total][self.mask]

    def free(self):
        self.mgk.free(self.p)


def _fields(dim, n, nz, k, seed):
    """w and k basis-like fields: mixed sign, each correlated with w (v_i . w is about N / 6 with sum |products| about N / 3)"""
    rng = np.random.default_rng(seed)
    N = n * n * (nz if dim == 3 else 1)
    w = rng.uniform(-1, 1, N)
    v = [rng.uniform(-1, 1, N) + 0.5 * w for _ in range(k)]
    return w, v


def _close(got, exact):
    return abs(got - exact) <= 1e-13 * abs(exact)


@pytest.mark.parametrize("dim,n,nz,k,policy", SHAPES)
def test_orthogonalisation_passes(mgk, orc, dim, n, nz, k, policy):
    L = mgk.L
    g = _geom(mgk, dim, n, nz)
    w, v = _fields(dim, n, nz, k, 100 * n + 10 * k + dim)
    dv = [mgk.to_field(g, x) for x in v]
    # w carries sentinels in its ghosts: the sums must skip them and the update must leave them
    dw = Sentinel(mgk, g, w)
    hdev = mgk.alloc(8 * KMAX)
    out = (C.c_double * k)()
    L.mgk_set_tuning(policy, -1)
    try:
        # ---- all k dots in one pass, delivered at once
        mgk._chk(L.mgk_multi_dot_f64(mgk.ctx, C.byref(g), k, _ptrs(dv), dw.p, hdev, out, None))
        h = np.array(out[:])
        assert np.array_equal(mgk.download(hdev, k), h)                 # device memory and the landing area hold the same values
        for i in range(k):
            assert _close(h[i], math.fsum(v[i] * w)), (i, h[i], math.fsum(v[i] * w))
        # ---- the update reads h from device memory; nothing is delivered until the fetch
        mgk._chk(L.mgk_multi_dot_f64(mgk.ctx, C.byref(g), k, _ptrs(dv), dw.p, hdev, None, None))
        mgk._chk(L.mgk_multi_axpy_sumsq_f64(mgk.ctx, C.byref(g), k, hdev, _ptrs(dv), dw.p, None, None))
        h2, ss = (C.c_double * k)(), C.c_double()
        mgk._chk(L.mgk_krylov_fetch(mgk.ctx, k, h2, C.byref(ss), None))
        assert np.array_equal(np.array(h2[:]), h)                       # deterministic: the same bits as the first pass
        ref = w.copy()
        for i in range(k):
            ref = ref - h[i] * v[i]
        got = dw.interior()
        assert np.array_equal(got, ref)
        assert _close(ss.value, math.fsum(ref * ref)), (ss.value, math.fsum(ref * ref))
        # ---- A (the updated field) through the product's stencil kernel equals the oracle's: the ghosts it reads are zero
        wz = mgk.to_field(g, got)
        mgk._chk(L.mgk_multi_dot_f64(mgk.ctx, C.byref(g), k, _ptrs(dv), wz, hdev, None, None))
        mgk._chk(L.mgk_multi_axpy_sumsq_f64(mgk.ctx, C.byref(g), k, hdev, _ptrs(dv), wz, C.byref(ss), None))
        h3 = mgk.download(hdev, k)
        ref2 = ref.copy()
        for i in range(k):
            ref2 = ref2 - h3[i] * v[i]
        As = orc.level_stencil(dim, n + 2, 0)[0]
        y = mgk.field(g)
        mgk._chk(L.mgk_apply_f64(mgk.ctx, C.byref(g), mgk.coef(As), wz, y, None))
        mgk.sync()
        assert np.array_equal(mgk.from_field(g, y), orc.apply(dim, n, As, ref2, nz=nz if dim == 3 else None))
        mgk.free(wz); mgk.free(y)
    finally:
        L.mgk_set_tuning(-1, -1)
        for f in dv:
            mgk.free(f)
        dw.free(); mgk.free(hdev)


@pytest.mark.parametrize("dim,n,nz,k,policy", SHAPES)
def test_lincomb_and_scale_to(mgk, dim, n, nz, k, policy):
    L = mgk.L
    g = _geom(mgk, dim, n, nz)
    w, v = _fields(dim, n, nz, k, 7 + 100 * n + 10 * k + dim)
    y = np.random.default_rng(n + k).uniform(-2, 2, k)
    dv = [mgk.to_field(g, x) for x in v]
    L.mgk_set_tuning(policy, -1)
    try:
        o = Sentinel(mgk, g)
        mgk._chk(L.mgk_lincomb_f64(mgk.ctx, C.byref(g), k, (C.c_double * k)(*y), _ptrs(dv), o.p, None))
        mgk.sync()
        ref = y[0] * v[0]
        for i in range(1, k):
            ref = ref + y[i] * v[i]
        assert np.array_equal(o.interior(), ref)
        o.free()
        # out = a x into one destination, into two, and in place
        a = 1.0 / 3.0
        o1, o2 = Sentinel(mgk, g), Sentinel(mgk, g)
        mgk._chk(L.mgk_scale_to_f64(mgk.ctx, C.byref(g), a, dv[0], o1.p, None, None))
        mgk.sync()
        assert np.array_equal(o1.interior(), a * v[0])
        assert np.all(mgk.download(o2.p, g.total) == SENT)
        mgk._chk(L.mgk_scale_to_f64(mgk.ctx, C.byref(g), -a, dv[0], o1.p, o2.p, None))
        mgk.sync()
        assert np.array_equal(o1.interior(), -a * v[0]) and np.array_equal(o2.interior(), -a * v[0])
        mgk._chk(L.mgk_scale_to_f64(mgk.ctx, C.byref(g), 3.0, o1.p, o1.p, None, None))
        mgk.sync()
        assert np.array_equal(o1.interior(), 3.0 * (-a * v[0]))
        o1.free(); o2.free()
    finally:
        L.mgk_set_tuning(-1, -1)
        for f in dv:
            mgk.free(f)


def test_refusals(mgk):
    """k outside 1 .. MGK_KRYLOV_MAX, a null operand, an output among the operands, and a geometry of even width (n = 2): no launch"""
    from multigrid_petsc_amd.mgk import Geom
    L = mgk.L
    g = mgk.geom(2, 15)
    f = [mgk.field(g) for _ in range(3)]
    h = mgk.alloc(8 * KMAX)
    two = (C.c_double * 2)(1.0, 1.0)
    assert L.mgk_multi_dot_f64(mgk.ctx, C.byref(g), 0, _ptrs(f[:2]), f[2], h, None, None) != 0
    assert L.mgk_multi_dot_f64(mgk.ctx, C.byref(g), KMAX + 1, _ptrs(f[:2]), f[2], h, None, None) != 0
    assert L.mgk_multi_dot_f64(mgk.ctx, C.byref(g), 2, (C.c_void_p * 2)(f[0].value, None), f[2], h, None, None) != 0
    assert L.mgk_multi_axpy_sumsq_f64(mgk.ctx, C.byref(g), 2, h, _ptrs(f[:2]), f[1], None, None) != 0
    assert L.mgk_lincomb_f64(mgk.ctx, C.byref(g), 2, two, _ptrs(f[:2]), f[0], None) != 0
    assert L.mgk_scale_to_f64(mgk.ctx, C.byref(g), 2.0, f[0], f[1], f[1], None) != 0
    assert L.mgk_krylov_fetch(mgk.ctx, KMAX + 1, two, None, None) != 0
    even = Geom()
    assert L.mgk_geom_init(C.byref(even), 2, 2, 2, 1) != 0
    C.memmove(C.byref(even), C.byref(g), C.sizeof(Geom))
    even.nx = 2
    assert L.mgk_multi_dot_f64(mgk.ctx, C.byref(even), 2, _ptrs(f[:2]), f[2], h, None, None) != 0
    from multigrid_petsc_amd.mgk import MgkError
    with pytest.raises(MgkError, match="mgk_scale_to_f64"):
        mgk._chk(L.mgk_scale_to_f64(mgk.ctx, C.byref(even), 2.0, f[0], f[1], None, None))
    for p in f + [h]:
        mgk.free(p)
