"""The four passes of the x-line sweep in chunks (csrc/mgk_xline_chunk.hip) against tests/xchunkline_reference.py, in the manner of
tests/test_chunkline_kernels_gpu.py: mgk_xline_chunk_forward_f64, _backward_, _reduce_ and _correct_.

  outputs        np.array_equal on what every pass leaves in memory: t (z with the residual r_s in the separator columns, then x' on the chunk
                 columns), the separator workspace sep (R after the forward pass, XL and XR after the backward pass, XI after the reduction)
                 and u' (the kernels follow the reference operation for operation, no FMA)
  fields         uniform(-1, 1), laid out by hand (offset = org + i pitch + j), so that even widths can be run too
  interior only  every field -- inputs included -- starts from a sentinel on the ghost ring, the padding and 256 doubles past the field, sep
                 from a sentinel everywhere and 256 doubles past it, the tables carry a sentinel in their padding: the outputs keep it wherever
                 the definition writes nothing (XR[K-1] when the last column is a separator included), and the results show that no input's
                 ghost ring or padding was used
  forms          from a guess and from the zero guess (u = NULL), unew == u and unew != u
  columns        nx = 1, 15 .. 17, 31 .. 33, 48, 63 .. 65, 96, 127 .. 129, 255: below, at and above the tile of 16 columns and the 128 columns of
                 a wave of the correction; nx = K c (an empty last chunk, the last column a separator) and nx = K c + 1 (a last chunk of one column)
  rows           ny = 1, 2, 61 .. 65, 125, 130 (the forward tile stores 62 rows per wave, the backward tile and the reduction 64, the correction
                 16), with every nx: square and rectangular both ways
  periods        c = 16, 32, 48, 64, 256; with c = 256 there is no separator and the four passes give the bits of mgk_xline_forward_f64 +
                 mgk_xline_backward_f64
  tables         tests/row_tables._rt_tables, tests/coef_cases.distinct_row_tables (W != E, S != N, varying with the row; ny x nx tables at a
                 stride of nx rounded up to 16) and levels of meshes 0 / 1 / 2 from the oracle's assembled rows, mesh 0 in the stride-0 form
  store policy   both forced forms (mgk_set_tuning(variant = 0 / 1)) and the choice by size
  refusals       3-D geometry, c not a positive multiple of 16, aliasing, strides"""
import ctypes as C

import numpy as np
import pytest

import line_reference as LR
import xchunkline_reference as XC
import xline_reference as XR
from oracle import Oracle
from coef_cases import distinct_row_tables
from row_tables import _rt_tables

pytestmark = pytest.mark.gpu
SENT = 12345.678
NXS = [1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 127, 128, 129, 255]
NYS = [1, 2, 61, 62, 63, 64, 65, 125, 130]
PERIODS = [16, 32, 48, 64, 256]
# (npts, level, mesh): n = 63 (uniform: stride 0), 63, 63, 31, 127 (uniform), 255, 255 (uniform)
MESH_LEVELS = [(65, 0, 0), (65, 0, 1), (129, 1, 2), (33, 0, 1), (129, 0, 0), (257, 0, 2), (257, 0, 0)]
PLANES = ("R", "XL", "XR", "XI")


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _geom(mgk, ny, nx):
    """the level geometry of a grid of ny rows and nx columns; an even nx borrows the padding of nx + 1 (the column past the interior is then
    a ghost column)"""
    g = mgk.geom(2, nx | 1, ny)
    g.nx = nx
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


def _strided(a, stride):
    """a table of a.shape[0] rows at a row stride (0: the first row serves all), a sentinel in the padding and past the end"""
    if stride == 0:
        return np.concatenate([a[0], np.full(8, SENT)])
    out = np.full((a.shape[0], stride), SENT)
    out[:, :a.shape[1]] = a
    return np.concatenate([out.ravel(), np.full(8, SENT)])


def _schur(a, sst):
    """SL / SG / SQ (ny x K) separator-major: entry [q sst + i]; sst = 0: entry [q]"""
    ny, K = a.shape
    if sst == 0:
        return np.concatenate([a[0], np.full(8, SENT)])
    out = np.full((K, sst), SENT)
    out[:, :ny] = a.T
    return np.concatenate([out.ravel(), np.full(8, SENT)])


def _sep_image(sep, K, ny):
    """the workspace as the kernels lay it out, the sentinel wherever the reference has formed nothing"""
    ss = (ny + 15) // 16 * 16
    raw = np.full(4 * K * ss + 256, SENT)
    for p, name in enumerate(PLANES):
        for q in range(K):
            row = sep[name][q]
            if not np.any(np.isnan(row)):
                raw[(p * K + q) * ss:(p * K + q) * ss + ny] = row
    return raw


def _run(mgk, ny, nx, c, ct, seed, policy=-1, uniform=False):
    """ny rows (ct is ny x 5) by nx columns; uniform: every row of ct is the same and the tables take the stride-0 form"""
    L = mgk.L
    g = _geom(mgk, ny, nx)
    rng = np.random.default_rng(seed)
    b, u = rng.uniform(-1, 1, (ny, nx)), rng.uniform(-1, 1, (ny, nx))
    scale = 0.8
    tab = XC.tables(ct, c, nx)
    K = tab["K"]
    gs = 0 if uniform else (nx + 15) // 16 * 16
    sst = 0 if uniform else (ny + 15) // 16 * 16
    if uniform:
        assert all(np.array_equal(ct[i], ct[0]) for i in range(ny))
    dct = mgk.upload(ct)
    d = {k: mgk.upload(_strided(tab[k], gs)) for k in ("g", "v", "w")}
    d.update({k: mgk.upload(_schur(tab[k], sst)) for k in ("SL", "SG", "SQ")})
    db, du = _put(mgk, g, b), _put(mgk, g, u)
    G = C.byref(g)
    ptrs = [dct, db, du] + list(d.values())
    nsep = 4 * K * ((ny + 15) // 16 * 16) + 256
    L.mgk_set_tuning(policy, -1)
    try:
        for guess in (True, False):
            uin, uref = (du, u) if guess else (None, None)
            tag = (ny, nx, c, guess)
            dt, ds = _put(mgk, g, None), mgk.upload(np.full(nsep, SENT))
            ptrs += [dt, ds]
            tref, sref = XC.forward(ct, tab, b, uref)
            mgk._chk(L.mgk_xline_chunk_forward_f64(mgk.ctx, G, c, dct, d["g"], gs, db, uin, dt, ds, None))
            mgk.sync()
            assert np.array_equal(_get(mgk, g, dt), tref), ("z", tag)
            zref = tref
            assert np.array_equal(mgk.download(ds, nsep), _sep_image(sref, K, ny)), ("R", tag)
            tref, sref = XC.backward(ct, tab, tref, sref)
            mgk._chk(L.mgk_xline_chunk_backward_f64(mgk.ctx, G, c, dct, d["g"], gs, dt, ds, None))
            mgk.sync()
            assert np.array_equal(_get(mgk, g, dt), tref), ("x'", tag)
            assert np.array_equal(mgk.download(ds, nsep), _sep_image(sref, K, ny)), ("XL, XR", tag)
            sref = XC.reduce(ct, tab, sref, nx)
            mgk._chk(L.mgk_xline_chunk_reduce_f64(mgk.ctx, G, c, dct, d["SL"], d["SG"], d["SQ"], sst, ds, None))
            mgk.sync()
            assert np.array_equal(mgk.download(ds, nsep), _sep_image(sref, K, ny)), ("XI", tag)
            oref = XC.correct(tab, scale, tref, sref, uref)
            do = _put(mgk, g, None)
            ptrs.append(do)
            mgk._chk(L.mgk_xline_chunk_correct_f64(mgk.ctx, G, c, d["v"], d["w"], gs, scale, dt, ds, uin, do, None))
            mgk.sync()
            assert np.array_equal(_get(mgk, g, do), oref), ("unew", tag)
            assert np.array_equal(_get(mgk, g, dt), tref), ("the correction changed t", tag)
            assert np.array_equal(mgk.download(ds, nsep), _sep_image(sref, K, ny)), ("the correction changed sep", tag)
            if guess:
                # in place (the normal use): u' lands in u, whose surroundings stay as they were
                da = _put(mgk, g, u)
                ptrs.append(da)
                mgk._chk(L.mgk_xline_chunk_correct_f64(mgk.ctx, G, c, d["v"], d["w"], gs, scale, dt, ds, da, da, None))
                mgk.sync()
                assert np.array_equal(_get(mgk, g, da), oref), ("in place", tag)
            if K == 0:
                # no separator: the bits of the two plain passes, on the plain table
                dg = mgk.upload(_strided(XR.table(ct, nx), gs))
                dp, dq = _put(mgk, g, None), _put(mgk, g, None)
                ptrs += [dg, dp, dq]
                mgk._chk(L.mgk_xline_forward_f64(mgk.ctx, G, dct, dg, gs, db, uin, dp, None))
                mgk._chk(L.mgk_xline_backward_f64(mgk.ctx, G, dct, dg, gs, scale, dp, uin, dq, None))
                mgk.sync()
                assert np.array_equal(_get(mgk, g, dp), zref) and np.array_equal(_get(mgk, g, dq), oref), ("plain passes", tag)
        assert np.array_equal(_get(mgk, g, db), b) and np.array_equal(_get(mgk, g, du), u)     # the inputs are untouched
    finally:
        L.mgk_set_tuning(-1, -1)
        for p in ptrs:
            mgk.free(p)


@pytest.mark.parametrize("nx", NXS)
def test_xchunk_passes_on_non_symmetric_row_tables(mgk, nx):
    """every coefficient of a row distinct and varying with the row (W != E: a swapped x neighbour shows; S != N), ny x nx tables; every ny
    with every nx: square where they meet, rectangular both ways otherwise"""
    for ny in NYS:
        ct = distinct_row_tables(np.random.default_rng(4000 + 7 * nx + ny), ny)[0]
        for c in PERIODS:
            _run(mgk, ny, nx, c, ct, 11 * nx + ny + c)


@pytest.mark.parametrize("n", NXS)
def test_xchunk_passes_on_random_row_tables(mgk, n):
    ct = _rt_tables(np.random.default_rng(1000 + n), n)[0]
    for c in PERIODS:
        _run(mgk, n, n, c, ct, 7 * n + c)


@pytest.mark.parametrize("npts,level,mesh", MESH_LEVELS)
def test_xchunk_passes_on_level_tables(mgk, orc, npts, level, mesh):
    ct = LR.level_table(orc, npts, level, mesh)
    n = ct.shape[0]
    if mesh == 0:
        ct = np.tile(ct[min(1, n - 1)], (n, 1))         # the product's uniform table: the level's five constants in every row
    for c in PERIODS:
        _run(mgk, n, n, c, ct, npts + 10 * level + mesh + c, uniform=(mesh == 0))


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("nx", [17, 64, 129, 255])
def test_both_store_policies(mgk, nx, policy):
    for ny in (2, 63, 130):
        ct = distinct_row_tables(np.random.default_rng(3000 + nx + ny), ny)[0]
        for c in (16, 48, 256):
            _run(mgk, ny, nx, c, ct, 5 * nx + policy + c + ny, policy=policy)


def test_refusals(mgk):
    """2-D only; c a positive multiple of 16; the scratch field aliasing b, u or sep, unew aliasing the scratch field; a pitch above 2^21
    doubles; a stride below the width, above 2^21 doubles or (the spikes) odd; no workspace where there is a separator"""
    L = mgk.L
    g, g3 = _geom(mgk, 7, 33), mgk.geom(3, 7)
    t = mgk.upload(np.ones(4096))
    f, f2, f3 = _put(mgk, g, None), _put(mgk, g, None), _put(mgk, g, None)
    G, G3 = C.byref(g), C.byref(g3)
    big = (1 << 21) + 16

    def four(Gx, c, gs=48, sst=16, sep=t):
        return (L.mgk_xline_chunk_forward_f64(mgk.ctx, Gx, c, t, t, gs, f, None, f2, sep, None),
                L.mgk_xline_chunk_backward_f64(mgk.ctx, Gx, c, t, t, gs, f, sep, None),
                L.mgk_xline_chunk_reduce_f64(mgk.ctx, Gx, c, t, t, t, t, sst, sep, None),
                L.mgk_xline_chunk_correct_f64(mgk.ctx, Gx, c, t, t, gs, 0.8, f, sep, None, f2, None))

    assert all(rc != 0 for rc in four(G3, 16))
    for c in (0, -16, 8, 24, 17):
        assert all(rc != 0 for rc in four(G, c)), c
    assert all(rc != 0 for rc in four(G, 16, gs=big, sst=big))
    assert all(rc != 0 for rc in four(G, 16, gs=32, sst=6))              # strides below the width / the height
    wide = _geom(mgk, 7, 33)
    wide.pitch = (1 << 21) + 16                                         # a pitch no window can address: refused before any launch
    assert all(rc != 0 for rc in four(C.byref(wide), 16))
    assert all(rc != 0 for rc in four(G, 16, sep=None))                 # nx >= c: there is a separator
    assert L.mgk_xline_chunk_correct_f64(mgk.ctx, G, 16, t, t, 49, 0.8, f, t, None, f2, None) != 0          # an odd stride of the spikes
    assert L.mgk_xline_chunk_forward_f64(mgk.ctx, G, 16, t, t, 48, f, None, f, t, None) != 0                 # t aliases b
    assert L.mgk_xline_chunk_forward_f64(mgk.ctx, G, 16, t, t, 48, f, f2, f2, t, None) != 0                  # t aliases u
    assert L.mgk_xline_chunk_forward_f64(mgk.ctx, G, 16, t, t, 48, f, f2, f3, f3, None) != 0                 # t aliases sep
    assert L.mgk_xline_chunk_backward_f64(mgk.ctx, G, 16, t, t, 48, f, f, None) != 0
    assert L.mgk_xline_chunk_correct_f64(mgk.ctx, G, 16, t, t, 48, 0.8, f, t, None, f, None) != 0            # unew aliases t
    assert L.mgk_xline_chunk_forward_f64(mgk.ctx, G, 16, None, t, 48, f, f2, f3, t, None) != 0
    with pytest.raises(Exception, match="mgk_xline_chunk_correct_f64"):
        mgk._chk(L.mgk_xline_chunk_correct_f64(mgk.ctx, G3, 16, t, t, 48, 0.8, f, t, None, f2, None))
    for p in (t, f, f2, f3):
        mgk.free(p)
