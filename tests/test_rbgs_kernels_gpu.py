"""The red-black Gauss-Seidel kernels (csrc/mgk_rbgs.hip) against tests/rbgs_reference.py: mgk_rbgs_2d_f64 and mgk_prolong_rbgs_2d_f64.

  outputs        np.array_equal on unew (the kernels follow the reference operation for operation, no FMA)
  fields         uniform(-1, 1); fields are laid out by hand (offset = org + i pitch + j), so that even widths can be run too:
                 mgk_geom_init knows only the odd widths of level grids, the plain form takes any
  interior only  unew starts from a sentinel pattern (ghost ring, padding and 256 doubles past the field): everything outside the
                 interior keeps it
  widths         1, 2, 3; 119 .. 121 (a wave stores 120 columns with nsweeps = 2) and 123 .. 125 (124 with nsweeps = 1); 241, 255 (three waves)
  heights        1, 2, 5; L - 1, L, L + 1, 2 L + 3 for the chunk length L = 12 of small fields; a chunk length given by the knob (6; 5, rounded to 6)
  forms          nsweeps 1 and 2; from a guess and from the zero guess (u = NULL); constants (a level stencil, and five distinct values of
                 mixed sign: tests/coef_cases.distinct_coef) and row tables (coef_cases.distinct_row_tables: W != E and S != N, so a
                 swapped neighbour or a swapped colour shows); both store policies (mgk_set_tuning(variant = 0 / 1))
  prolongation   equal to mgk_prolong_add_f64 followed by the plain pass, and to the reference over the oracle's prolongation, on the pairs
                 255 / 127 and 121 / 60
  refusals       nsweeps other than 1 or 2, unew == u, unew == b, no u with the prolongation, a coarse grid that does not match, ctab without dtab"""
import ctypes as C

import numpy as np
import pytest

import rbgs_reference as RB
from coef_cases import distinct_coef, distinct_row_tables
from oracle import Oracle

pytestmark = pytest.mark.gpu
SENT = 12345.678
LCHUNK = 12                                      # the kernel's chunk length on fields too small to fill the GPU (csrc/mgk_rbgs.hip: rbgs_2d)
WIDTHS = [1, 2, 3, 119, 120, 121, 123, 124, 125, 241, 255]
HEIGHTS = [1, 2, 5, LCHUNK - 1, LCHUNK, LCHUNK + 1, 2 * LCHUNK + 3]
SCALE = 0.8


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _geom(mgk, nx, ny):
    """the geometry of an ny x nx field; an even nx borrows the padding of nx + 1 (the column past the interior is then a ghost column)"""
    g = mgk.geom(2, nx | 1, ny)
    g.nx = nx
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


def _operators(mgk, orc, rng, ny):
    """[(name, coef argument, dinv, device ctab, device dtab, reference tables)]: two constant sets and one pair of row tables"""
    ops = []
    for name, As in (("level", orc.level_stencil(2, 65, 1)[0]), ("distinct", distinct_coef(rng, 2))):
        dinv = 1.0 / float(As[2])
        ops.append((name, mgk.coef(list(As)), dinv, None, None, RB.const_table(As, dinv, ny)))
    ct, dt = distinct_row_tables(rng, ny)
    assert np.all(ct[:, 0] != ct[:, 4])
    ops.append(("tables", None, 1.0, mgk.upload(ct), mgk.upload(dt), (ct, dt)))
    return ops


def _run_plain(mgk, orc, nx, ny, seed, zchunk=-1):
    L = mgk.L
    g = _geom(mgk, nx, ny)
    G = C.byref(g)
    rng = np.random.default_rng(seed)
    b, u = rng.uniform(-1, 1, (ny, nx)), rng.uniform(-1, 1, (ny, nx))
    db, du = _put(mgk, g, b), _put(mgk, g, u)
    ops = _operators(mgk, orc, rng, ny)
    try:
        for name, coef, dinv, dct, ddt, (ct, dt) in ops:
            for ns in (1, 2):
                for guess in (True, False):
                    want = RB.sweeps(ct, dt, SCALE, b, u if guess else None, ns)
                    for policy in (0, 1):
                        L.mgk_set_tuning(policy, zchunk)
                        do = _put(mgk, g, None, SENT)
                        mgk._chk(L.mgk_rbgs_2d_f64(mgk.ctx, G, coef, dinv, SCALE, dct, ddt, ns, db, du if guess else None, do, None))
                        mgk.sync()
                        got = _get(mgk, g, do, SENT)
                        mgk.free(do)
                        assert np.array_equal(got, want), (nx, ny, name, ns, guess, policy, float(np.abs(got - want).max()))
    finally:
        L.mgk_set_tuning(-1, -1)
        for p in [db, du] + [q for op in ops for q in op[3:5] if q is not None]:
            mgk.free(p)


@pytest.mark.parametrize("nx", WIDTHS)
def test_rbgs_pass_equals_the_reference(mgk, orc, nx):
    for ny in HEIGHTS:
        _run_plain(mgk, orc, nx, ny, seed=1000 * nx + ny)


@pytest.mark.parametrize("zchunk", [6, 5, 2])
def test_rbgs_pass_with_a_given_chunk_length(mgk, orc, zchunk):
    """the second knob of mgk_set_tuning: chunks of that many rows, rounded up to even; seams every few rows"""
    for nx, ny in ((125, 27), (241, 13)):
        _run_plain(mgk, orc, nx, ny, seed=77 + zchunk, zchunk=zchunk)


@pytest.mark.parametrize("nf", [255, 121])
def test_prolongation_form_equals_prolong_add_and_the_plain_pass(mgk, orc, nf):
    L = mgk.L
    nc = (nf - 1) // 2
    gf, gc = mgk.geom(2, nf), _geom(mgk, nc, nc)
    GF, GC = C.byref(gf), C.byref(gc)
    rng = np.random.default_rng(nf)
    b, u, uc = rng.uniform(-1, 1, (nf, nf)), rng.uniform(-1, 1, (nf, nf)), rng.uniform(-1, 1, (nc, nc))
    db, du, duc = _put(mgk, gf, b), _put(mgk, gf, u), _put(mgk, gc, uc)
    # u + P uc: by the product's own prolongation, which must equal the oracle's
    dsum = _put(mgk, gf, u)
    mgk._chk(L.mgk_prolong_add_f64(mgk.ctx, GF, GC, duc, dsum, None))
    mgk.sync()
    usum = _get(mgk, gf, dsum, 0.0)
    assert np.array_equal(usum.ravel(), orc.prolong_add(2, nf, uc.ravel().copy(), u.ravel().copy()))
    ops = _operators(mgk, orc, rng, nf)
    try:
        for name, coef, dinv, dct, ddt, (ct, dt) in ops:
            for ns in (1, 2):
                want = RB.sweeps(ct, dt, SCALE, b, usum, ns)
                for policy in (0, 1):
                    L.mgk_set_tuning(policy, -1)
                    outs = []
                    for fused in (True, False):
                        do = _put(mgk, gf, None, SENT)
                        if fused:
                            mgk._chk(L.mgk_prolong_rbgs_2d_f64(mgk.ctx, GF, GC, coef, dinv, SCALE, dct, ddt, ns, db, duc, du, do, None))
                        else:
                            mgk._chk(L.mgk_rbgs_2d_f64(mgk.ctx, GF, coef, dinv, SCALE, dct, ddt, ns, db, dsum, do, None))
                        mgk.sync()
                        outs.append(_get(mgk, gf, do, SENT))
                        mgk.free(do)
                    assert np.array_equal(outs[0], outs[1]), (nf, name, ns, policy, float(np.abs(outs[0] - outs[1]).max()))
                    assert np.array_equal(outs[0], want), (nf, name, ns, policy, float(np.abs(outs[0] - want).max()))
    finally:
        L.mgk_set_tuning(-1, -1)
        for p in [db, du, duc, dsum] + [q for op in ops for q in op[3:5] if q is not None]:
            mgk.free(p)


def test_prolongation_form_on_short_and_odd_shapes(mgk, orc):
    """the prolongation with chunk seams and the wave tiles' edges: 13 x 125 from 6 x 62, 27 x 241 from 13 x 120, 5 x 247 from 2 x 123, 3 x 3 from 1 x 1; the reference
    prolongs by the product's mgk_prolong_add_f64 (pinned against the oracle above)"""
    L = mgk.L
    for nxf, nyf in ((125, 13), (241, 27), (247, 5), (3, 3)):
        gf, gc = mgk.geom(2, nxf, nyf), _geom(mgk, (nxf - 1) // 2, (nyf - 1) // 2)
        GF, GC = C.byref(gf), C.byref(gc)
        rng = np.random.default_rng(nxf + nyf)
        b, u, uc = rng.uniform(-1, 1, (nyf, nxf)), rng.uniform(-1, 1, (nyf, nxf)), rng.uniform(-1, 1, (gc.ny, gc.nx))
        db, du, duc, dsum = _put(mgk, gf, b), _put(mgk, gf, u), _put(mgk, gc, uc), _put(mgk, gf, u)
        mgk._chk(L.mgk_prolong_add_f64(mgk.ctx, GF, GC, duc, dsum, None))
        mgk.sync()
        usum = _get(mgk, gf, dsum, 0.0)
        ops = _operators(mgk, orc, rng, nyf)
        for name, coef, dinv, dct, ddt, (ct, dt) in ops:
            for ns in (1, 2):
                do = _put(mgk, gf, None, SENT)
                mgk._chk(L.mgk_prolong_rbgs_2d_f64(mgk.ctx, GF, GC, coef, dinv, SCALE, dct, ddt, ns, db, duc, du, do, None))
                mgk.sync()
                got = _get(mgk, gf, do, SENT)
                mgk.free(do)
                want = RB.sweeps(ct, dt, SCALE, b, usum, ns)
                assert np.array_equal(got, want), (nxf, nyf, name, ns, float(np.abs(got - want).max()))
        for p in [db, du, duc, dsum] + [q for op in ops for q in op[3:5] if q is not None]:
            mgk.free(p)


def test_bad_arguments_are_refused(mgk):
    L = mgk.L
    EINVAL = 10001
    gf, gc, gbad = mgk.geom(2, 31), mgk.geom(2, 15), mgk.geom(2, 13)
    GF, GC, GB = C.byref(gf), C.byref(gc), C.byref(gbad)
    coef = mgk.coef([1.0, 1.0, -4.0, 1.0, 1.0])
    db, du, do, duc = mgk.field(gf), mgk.field(gf), mgk.field(gf), mgk.field(gc)
    dct = mgk.upload(np.ones((31, 5)))
    try:
        for ns in (0, 3, -1):
            assert L.mgk_rbgs_2d_f64(mgk.ctx, GF, coef, -0.25, 1.0, None, None, ns, db, du, do, None) == EINVAL
            assert L.mgk_prolong_rbgs_2d_f64(mgk.ctx, GF, GC, coef, -0.25, 1.0, None, None, ns, db, duc, du, do, None) == EINVAL
        assert L.mgk_rbgs_2d_f64(mgk.ctx, GF, coef, -0.25, 1.0, None, None, 2, db, du, du, None) == EINVAL            # unew == u
        assert L.mgk_rbgs_2d_f64(mgk.ctx, GF, coef, -0.25, 1.0, None, None, 2, db, du, db, None) == EINVAL            # unew == b
        assert L.mgk_rbgs_2d_f64(mgk.ctx, GF, coef, -0.25, 1.0, None, None, 2, db, None, db, None) == EINVAL          # ... from the zero guess too
        assert L.mgk_rbgs_2d_f64(mgk.ctx, GF, None, -0.25, 1.0, None, None, 2, db, du, do, None) == EINVAL            # no coefficients
        assert L.mgk_rbgs_2d_f64(mgk.ctx, GF, None, -0.25, 1.0, dct, None, 2, db, du, do, None) == EINVAL             # ctab without dtab
        assert L.mgk_prolong_rbgs_2d_f64(mgk.ctx, GF, GC, coef, -0.25, 1.0, None, None, 2, db, duc, du, du, None) == EINVAL
        assert L.mgk_prolong_rbgs_2d_f64(mgk.ctx, GF, GC, coef, -0.25, 1.0, None, None, 2, db, duc, du, db, None) == EINVAL
        assert L.mgk_prolong_rbgs_2d_f64(mgk.ctx, GF, GC, coef, -0.25, 1.0, None, None, 2, db, duc, None, do, None) == EINVAL   # the prolongation reads u
        assert L.mgk_prolong_rbgs_2d_f64(mgk.ctx, GF, GB, coef, -0.25, 1.0, None, None, 2, db, duc, du, do, None) == EINVAL     # 31 is not 2 * 13 + 1
        mgk._chk(L.mgk_rbgs_2d_f64(mgk.ctx, GF, coef, -0.25, 1.0, None, None, 2, db, du, do, None))                   # the context still works
        mgk.sync()
    finally:
        for p in (db, du, do, duc, dct):
            mgk.free(p)
