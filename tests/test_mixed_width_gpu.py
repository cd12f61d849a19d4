"""The fp32 kernel INSTANCES of the mixed-precision cycle (BASELINE config 5) at headline width, against the CPU oracle's fp32 leg.

The fp32 fast paths switch on for full rows only: (nx + 1) % (64 * VX) == 0 with VX = 16 / sizeof(float) = 4 (row_shape_ok, j2zero_ok
and `full` in jacobi2<T>, mgk_kernels.hip), i.e. n = 255, 511, 1023 with 1, 2 and 4 waves per row.  test_mixed_gpu.py stops at n = 255,
the one-wave instance.  Here every fp32 entry point of the cycle runs on thin grids nx x ny x nz with nx = 1023 and 511 (nz = 3, 5, 9;
n = 255 as the control; a few ny != nx with (ny + 1) % 4 == 0) and is compared with the oracle (oracle/mgo_f32.c, thin forms
mgo_st_*_f32_thin): fields np.array_equal, ghosts zero, inputs unchanged.  No GPU result is compared with another GPU result.  On the
1023-wide cases the swept field also meets the float64 forward-error bound of tests/test_oracle.py, so a mismatch says by itself
whether the kernel or the oracle is off.

Which instance each entry point dispatches at nx = 511 / 1023 (W = 2 / 4 waves per row), and the test that pins it:
  mgk_jacobi_f32 / mgk_residual_f32   k_stencil<float,3,2,2,2,..> (variant 1, default at 511) / <float,3,4,2,2,..> (variant 2,
                                      default at 1023); variants 0 (<float,3,1,2,2>) and 3 (<float,3,4,1,4>) forced; the packed
                                      jac7 overload is the fp32 body of these                       test_sweeps_at_width
  mgk_jacobi_f32, tuning variant 34   k_jrow<float,W,..> (row form)                                  test_sweeps_at_width
  mgk_jacobi_zero_f32                 k_jacobi_zero<float>                                           test_sweeps_at_width
  mgk_jacobi2_f32                     k_jacobi2b<float,W,false> (default), k_jacobi2r<float,W,3> (variant 2),
                                      k_jacobi2<float,W,3> (variant 39), k_jacobi2<float,W,0> / k_jacobi2r<float,W,0> (36 / 37:
                                      predicated loads)                                               test_sweeps_at_width
  mgk_jacobi2_zero_f32                k_jacobi2b<float,W,true> (default), k_jacobi2<float,W,3,true> (variant 39)
                                                                                                     test_sweeps_at_width
  mgk_restrict_fw_f32                 k_restrict<float,3>                                            test_transfers_at_width
  mgk_prolong_add_f32                 k_prolong_add<float,3>                                         test_transfers_at_width
  mgk_prolong_jacobi_f32 (+ _range)   k_pjrow<float,W,1,3> (default), <..,1,0> (31), <..,1,1> (33), <..,1,2> (35),
                                      k_stencil<float,..,MODE_PJACOBI> (30: LDS tile)                 test_transfers_at_width, slabs
  mgk_residual_restrict_f32 / _jz_f32 / _range_f32 / _slab_f32
                                      k_rrrow<float,W,1,2> (default), <..,1,0> (31), k_resrestrict<float,W> (30)
                                                                                                     test_transfers_at_width, slabs
  mgk_restrict_finish_f32             k_restrict_finish<float>                                       test_fp32_slab_forms
  mgk_jacobi2_slab_f32                k_jacobi2b<float,W,false> with far_lo / far_hi                 test_fp32_slab_forms
  mgk_jacobi_range_f32 / mgk_residual_range_f32   k_stencil<float,..> on plane ranges                test_fp32_slab_forms
  mgk_residual_f64_to_f32(_jz), mgk_correct_f64_from_f32, mgk_correct_residual_f64_f32(_jz)
                                      fp64 k_stencil / row kernels writing fp32                      test_bridges_at_width
Whole runs: a 511^3 mixed solve, four loopback slab ranks at 511^3 and two cycles at 1023^3 (where the host has the memory), each
against mgo_vcycle_mixed."""
import ctypes as C

import numpy as np
import pytest

from oracle import Oracle

pytestmark = pytest.mark.gpu
SCALE = 6.0 / 7.0
U32 = 2.0 ** -24
RED_RTOL = 1e-13

SHAPES = [(1023, 1023, 3), (1023, 1023, 5), (1023, 1023, 9), (511, 511, 3), (511, 511, 5), (511, 511, 9), (255, 255, 5),
          (1023, 7, 9), (1023, 11, 5), (511, 11, 7)]
SQUARE = [s for s in SHAPES if s[0] == s[1]]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _geom32(mgk, nx, ny, nz):
    from multigrid_petsc_amd.mgk import Geom
    g = Geom()
    mgk._chk(mgk.L.mgk_geom_init_f32(C.byref(g), 3, nx, ny, nz))
    return g


def _raw32(mgk, g, f):
    out = np.empty(g.total, dtype=np.float32)
    mgk._chk(mgk.L.mgk_d2h(mgk.ctx, out.ctypes.data_as(C.c_void_p), f, out.nbytes))
    return out


def _upload32(mgk, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float32)
    p = mgk.alloc(arr.nbytes)
    mgk._chk(mgk.L.mgk_h2d(mgk.ctx, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes))
    return p


def _padded32(g, planes):
    """padded fp32 array of geometry g; planes: {local plane index (-1 .. nz): (ny, nx) array}"""
    pad = np.zeros(g.total, dtype=np.float32)
    for k, pl in planes.items():
        for i in range(g.ny):
            o = g.org + k * g.plane + i * g.pitch
            pad[o:o + g.nx] = pl[i]
    return pad


class Thin32:
    """seeded fp32 fields on an nx x ny x nz grid and its coarse grid, on the device and on the host"""

    def __init__(self, mgk, orc, nx, ny, nz, seed):
        self.mgk, self.orc, self.nx, self.ny, self.nz = mgk, orc, nx, ny, nz
        self.nxc, self.nyc, self.nzc = (nx - 1) // 2, (ny - 1) // 2, (nz - 1) // 2
        rng = np.random.default_rng(seed)
        self.As = orc.level_stencil(3, nx + 2, 0)[0]
        self.Asc = orc.level_stencil(3, self.nxc + 2, 0)[0]
        self.dinv, self.dinvc = 1.0 / self.As[3], 1.0 / self.Asc[3]
        N, Nc = nx * ny * nz, self.nxc * self.nyc * self.nzc
        f32 = lambda m: rng.uniform(-1, 1, m).astype(np.float32)
        self.u, self.b, self.uc = f32(N), f32(N), f32(Nc)
        self.g, self.gc = _geom32(mgk, nx, ny, nz), _geom32(mgk, self.nxc, self.nyc, self.nzc)
        self.du, self.db, self.duc = mgk.to_field32(self.g, self.u), mgk.to_field32(self.g, self.b), mgk.to_field32(self.gc, self.uc)
        self.coef = mgk.coef(self.As)
        self._own = [self.du, self.db, self.duc]

    # oracle operators on the thin grid (fp32 leg)
    def J(self, u, zero_guess=False):
        return self.orc.jacobi32(self.nx, self.As, SCALE, self.b, u, zero_guess=zero_guess, nz=self.nz, ny=self.ny)

    def res(self, u):
        return self.orc.residual32(self.nx, self.As, self.b, u, nz=self.nz, ny=self.ny)

    def R(self, r):
        return self.orc.restrict32(self.nx, r, nzf=self.nz, nzc=self.nzc, nyf=self.ny)

    def P(self, uc, u):
        return self.orc.prolong_add32(self.nx, uc, u, nzf=self.nz, nzc=self.nzc, nyf=self.ny)

    def Jc0(self, bc):
        """the coarse level's first sweep from the zero guess"""
        return self.orc.jacobi32(self.nxc, self.Asc, SCALE, bc, np.zeros_like(bc), zero_guess=True, nz=self.nzc, ny=self.nyc)

    def out(self, coarse=False):
        g = self.gc if coarse else self.g
        f = self.mgk.field32(g)                               # a fresh allocation is zero-filled; under tests/guarded.py its interior is poisoned
        self._own.append(f)
        return f

    def get(self, f, coarse=False):
        return self.mgk.from_field32(self.gc if coarse else self.g, f)

    def ghosts_clean(self, f, coarse=False):
        g = self.gc if coarse else self.g
        raw, inner = _raw32(self.mgk, g, f), self.get(f, coarse)
        return np.count_nonzero(raw) == np.count_nonzero(inner)

    def inputs_untouched(self):
        return (np.array_equal(self.get(self.du), self.u) and np.array_equal(self.get(self.db), self.b)
                and np.array_equal(self.get(self.duc, True), self.uc))

    def close(self):
        for p in self._own:
            self.mgk.free(p)


def _where(got, want, nx, ny):
    """first mismatching unknowns: (plane, row, column, lane = column // 4, wave = lane // 64, at a wave seam)"""
    bad = np.flatnonzero(got != want)[:6]
    out = []
    for q in bad:
        k, rem = divmod(int(q), nx * ny)
        i, j = divmod(rem, nx)
        lane = (j + 1) // 4                   # the row kernels' lane owns columns 4 lane - 1 .. 4 lane + 2
        out.append((k, i, j, lane, lane // 64, lane % 64 in (0, 63)))
    return f"{np.count_nonzero(got != want)} mismatches, first (k, i, j, lane, wave, seam): {out}"


def _eq(got, want, t, what):
    assert np.array_equal(got, want), f"{what}: {_where(got, want, t.nx, t.ny)}"


def _sweep_bound(t, o, u):
    """the float64 forward-error bound of test_oracle.py::test_fp32_leg_within_its_forward_error_bound, on a kernel's sweep"""
    As32, d32 = Oracle.coef32(t.As)
    sd = float(np.float32(SCALE)) * float(d32)
    U = u.astype(np.float64).reshape(t.nz, t.ny, t.nx)
    Bv = t.b.astype(np.float64).reshape(U.shape)
    tt, S = np.zeros_like(U), np.zeros_like(U)
    terms = [(0, 1), (1, 1), (2, 1), None, (2, -1), (1, -1), (0, -1)]
    for q, sh in enumerate(terms):
        if sh is None:
            v = U
        else:
            ax, d = sh
            v = np.zeros_like(U)
            src, dst = [slice(None)] * 3, [slice(None)] * 3
            dst[ax], src[ax] = (slice(d, None), slice(None, -d)) if d > 0 else (slice(None, d), slice(-d, None))
            v[tuple(dst)] = U[tuple(src)]
        p = float(As32[q]) * v
        tt += p
        S += np.abs(p)
    ref = U + sd * (Bv - tt)
    err = np.abs(o.astype(np.float64).reshape(U.shape) - ref)
    return bool(np.all(err <= 16 * U32 * (np.abs(U) + abs(sd) * (np.abs(Bv) + S))))


@pytest.mark.parametrize("nx,ny,nz", SHAPES)
def test_sweeps_at_width(mgk, orc, nx, ny, nz):
    t = Thin32(mgk, orc, nx, ny, nz, 41000 + nx + ny + nz)
    L, g = mgk.L, C.byref(t.g)
    j1 = t.J(t.u)
    j2 = t.J(j1)
    r0 = t.res(t.u)
    jz = t.J(np.zeros_like(t.u), zero_guess=True)
    z3 = t.J(t.J(jz))
    if nx == 1023:
        assert _sweep_bound(t, j1, t.u), "the oracle's sweep is outside its float64 bound"
    for v in (-1, 0, 1, 2, 3, 34):
        for zc in (-1, 5):
            L.mgk_set_tuning(v, zc)
            o = t.out()
            mgk._chk(L.mgk_jacobi_f32(mgk.ctx, g, t.coef, t.dinv, SCALE, t.db, t.du, o, None))
            got = t.get(o)
            if nx == 1023 and not np.array_equal(got, j1):
                assert _sweep_bound(t, got, t.u), f"mgk_jacobi_f32 variant={v} zc={zc}: outside the float64 bound"
            _eq(got, j1, t, f"mgk_jacobi_f32 variant={v} zc={zc}")
            assert t.ghosts_clean(o)
            if v == 34:
                continue                                    # (the row form is a sweep-only form)
            o = t.out()
            mgk._chk(L.mgk_residual_f32(mgk.ctx, g, t.coef, t.db, t.du, o, None))
            _eq(t.get(o), r0, t, f"mgk_residual_f32 variant={v} zc={zc}")
            assert t.ghosts_clean(o)
    L.mgk_set_tuning(-1, -1)
    o = t.out()
    mgk._chk(L.mgk_jacobi_zero_f32(mgk.ctx, g, t.dinv, SCALE, t.db, o, None))
    _eq(t.get(o), jz, t, "mgk_jacobi_zero_f32")
    assert t.ghosts_clean(o)
    for v in (-1, 2, 36, 37, 39):
        for zc in (-1, 5):
            L.mgk_set_tuning(v, zc)
            o = t.out()
            mgk._chk(L.mgk_jacobi2_f32(mgk.ctx, g, t.coef, t.dinv, SCALE, t.db, t.du, o, None))
            _eq(t.get(o), j2, t, f"mgk_jacobi2_f32 variant={v} zc={zc}")
            assert t.ghosts_clean(o)
    for v in (-1, 39):
        L.mgk_set_tuning(v, -1)
        assert L.mgk_jacobi2_zero_ok_f32(g) == 1
        for zc in (-1, 5):
            L.mgk_set_tuning(v, zc)
            o = t.out()
            mgk._chk(L.mgk_jacobi2_zero_f32(mgk.ctx, g, t.coef, t.dinv, SCALE, t.db, o, None))
            _eq(t.get(o), z3, t, f"mgk_jacobi2_zero_f32 variant={v} zc={zc}")
            assert t.ghosts_clean(o)
    L.mgk_set_tuning(-1, -1)
    assert t.inputs_untouched()
    t.close()


@pytest.mark.parametrize("nx,ny,nz", SHAPES)
def test_transfers_at_width(mgk, orc, nx, ny, nz):
    t = Thin32(mgk, orc, nx, ny, nz, 42000 + nx + ny + nz)
    L, g, gc = mgk.L, C.byref(t.g), C.byref(t.gc)
    pu = t.P(t.uc, t.u)
    pj = t.J(pu)
    bc = t.R(t.res(t.u))
    bcu = t.R(t.u)
    jzc = t.Jc0(bc)
    assert np.abs(bc).max() > 0 and np.abs(jzc).max() > 0
    for v in (-1, 30, 31, 32, 33, 35):
        for zc in (-1, 5):
            L.mgk_set_tuning(v, zc)
            o = t.out()
            mgk._chk(L.mgk_prolong_jacobi_f32(mgk.ctx, g, gc, t.coef, t.dinv, SCALE, t.db, t.duc, t.du, o, None))
            _eq(t.get(o), pj, t, f"mgk_prolong_jacobi_f32 variant={v} zc={zc}")
            assert t.ghosts_clean(o)
            if v in (33, 35):
                continue                                    # (prolongation-only row forms)
            oc = t.out(coarse=True)
            mgk._chk(L.mgk_residual_restrict_f32(mgk.ctx, g, gc, t.coef, t.db, t.du, oc, None))
            _eq(t.get(oc, True), bc, t, f"mgk_residual_restrict_f32 variant={v} zc={zc}")
            assert t.ghosts_clean(oc, True)
            oc, ou = t.out(coarse=True), t.out(coarse=True)
            mgk._chk(L.mgk_residual_restrict_jz_f32(mgk.ctx, g, gc, t.coef, t.db, t.du, oc, ou, t.dinvc, SCALE, None))
            _eq(t.get(oc, True), bc, t, f"mgk_residual_restrict_jz_f32 variant={v} zc={zc}: coarse right-hand side")
            _eq(t.get(ou, True), jzc, t, f"mgk_residual_restrict_jz_f32 variant={v} zc={zc}: coarse zero-guess sweep")
            assert t.ghosts_clean(oc, True) and t.ghosts_clean(ou, True)
    L.mgk_set_tuning(-1, -1)
    oc = t.out(coarse=True)
    mgk._chk(L.mgk_restrict_fw_f32(mgk.ctx, g, gc, t.du, oc, None))
    _eq(t.get(oc, True), bcu, t, "mgk_restrict_fw_f32")
    assert t.ghosts_clean(oc, True)
    o = mgk.to_field32(t.g, t.u)                            # in place: on a copy of u
    t._own.append(o)
    mgk._chk(L.mgk_prolong_add_f32(mgk.ctx, g, gc, t.duc, o, None))
    _eq(t.get(o), pu, t, "mgk_prolong_add_f32")
    assert t.ghosts_clean(o)
    assert t.inputs_untouched()
    t.close()


@pytest.mark.parametrize("n,nz", [(s[0], s[2]) for s in SQUARE])
def test_bridges_at_width(mgk, orc, n, nz):
    """the fp64 <-> fp32 bridges of the outer step: fp32 and fp64 fields bit for bit, fp64 sums of squares to 1e-13"""
    rng = np.random.default_rng(43000 + n + nz)
    N = n * n * nz
    As = orc.level_stencil(3, n + 2, 0)[0]
    dinv = 1.0 / As[3]
    u, b, e = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(-1, 1, N).astype(np.float32)
    g, g32 = mgk.geom(3, n, n, nz), _geom32(mgk, n, n, nz)
    L, coef = mgk.L, mgk.coef(As)
    du, db, de = mgk.to_field(g, u), mgk.to_field(g, b), mgk.to_field32(g32, e)
    own = [du, db, de]

    def f32():
        p = mgk.field32(g32)
        mgk._chk(L.mgk_memset0(mgk.ctx, p, 4 * g32.total, None))
        own.append(p)
        return p

    def f64():
        p = mgk.field(g)
        mgk._chk(L.mgk_memset0(mgk.ctx, p, 8 * g.total, None))
        own.append(p)
        return p

    def zsweep(r32):
        return orc.jacobi32(n, As, SCALE, r32, np.zeros_like(r32), zero_guess=True, nz=nz)

    r = orc.residual(3, n, As, b, u, nz=nz)
    ucorr = u + e.astype(np.float64)
    rc = orc.residual(3, n, As, b, ucorr, nz=nz)
    ss = C.c_double()
    for zc in (-1, 3):
        L.mgk_set_tuning(-1, zc)
        r32 = f32()
        mgk._chk(L.mgk_residual_f64_to_f32(mgk.ctx, C.byref(g), C.byref(g32), coef, db, du, r32, C.byref(ss), None))
        assert np.array_equal(mgk.from_field32(g32, r32), r.astype(np.float32)), f"mgk_residual_f64_to_f32 zc={zc}"
        assert abs(ss.value - orc.sumsq(r)) <= RED_RTOL * orc.sumsq(r)
        r32, e0 = f32(), f32()
        mgk._chk(L.mgk_residual_f64_to_f32_jz(mgk.ctx, C.byref(g), C.byref(g32), coef, db, du, r32, e0, dinv, SCALE, C.byref(ss), None))
        assert np.array_equal(mgk.from_field32(g32, r32), r.astype(np.float32)), f"mgk_residual_f64_to_f32_jz zc={zc}"
        assert np.array_equal(mgk.from_field32(g32, e0), zsweep(r.astype(np.float32))), f"mgk_residual_f64_to_f32_jz zc={zc}: e0"
        assert abs(ss.value - orc.sumsq(r)) <= RED_RTOL * orc.sumsq(r)
        un, r32 = f64(), f32()
        mgk._chk(L.mgk_correct_residual_f64_f32(mgk.ctx, C.byref(g), C.byref(g32), coef, db, du, de, un, r32, C.byref(ss), None))
        assert np.array_equal(mgk.from_field(g, un), ucorr), f"mgk_correct_residual_f64_f32 zc={zc}: corrected field"
        assert np.array_equal(mgk.from_field32(g32, r32), rc.astype(np.float32)), f"mgk_correct_residual_f64_f32 zc={zc}: residual"
        assert abs(ss.value - orc.sumsq(rc)) <= RED_RTOL * orc.sumsq(rc)
        un, r32, e0 = f64(), f32(), f32()
        mgk._chk(L.mgk_correct_residual_f64_f32_jz(mgk.ctx, C.byref(g), C.byref(g32), coef, db, du, de, un, r32, e0, dinv, SCALE,
                                                   C.byref(ss), None))
        assert np.array_equal(mgk.from_field(g, un), ucorr), f"mgk_correct_residual_f64_f32_jz zc={zc}: corrected field"
        assert np.array_equal(mgk.from_field32(g32, r32), rc.astype(np.float32)), f"mgk_correct_residual_f64_f32_jz zc={zc}: residual"
        assert np.array_equal(mgk.from_field32(g32, e0), zsweep(rc.astype(np.float32))), f"mgk_correct_residual_f64_f32_jz zc={zc}: e0"
        assert abs(ss.value - orc.sumsq(rc)) <= RED_RTOL * orc.sumsq(rc)
        raw = mgk.raw_field(g, un)
        assert np.count_nonzero(raw) == np.count_nonzero(ucorr)                 # ghosts of the corrected field stay zero
    L.mgk_set_tuning(-1, -1)
    assert np.array_equal(mgk.from_field(g, du), u) and np.array_equal(mgk.from_field(g, db), b)
    uc = mgk.to_field(g, u)
    own.append(uc)
    mgk._chk(L.mgk_correct_f64_from_f32(mgk.ctx, C.byref(g), C.byref(g32), de, uc, None))
    assert np.array_equal(mgk.from_field(g, uc), ucorr), "mgk_correct_f64_from_f32"
    assert np.array_equal(mgk.from_field32(g32, de), e)
    for p in own:
        mgk.free(p)


@pytest.mark.parametrize("n,nz,cuts", [
    (1023, 33, (0, 16)),                 # one slab: the whole grid through the slab entry points
    (1023, 33, (0, 5, 16)),              # uneven split
    (1023, 33, (0, 1, 15, 16)),          # a two-plane slab at the bottom, a three-plane slab at the top
    (511, 25, (0, 3, 4, 8, 12)),         # four ranks' worth: 6, 2, 8 and 9 planes
    (255, 63, (0, 7, 20, 31)),
    (255, 63, (0, 2, 29, 31)),
])
def test_fp32_slab_forms(mgk, orc, n, nz, cuts):
    """The fp32 slab and plane-range forms on z-slabs of a thin whole grid (coarse plane ranges `cuts`).  Every slab is given its
    neighbours' planes the way the halo exchange delivers them -- ghost planes of u and b, the far planes (lo: plane z0 - 2, hi:
    plane z1 + 1), the coarse u's ghost planes, the residual of the next slab's first plane -- runs the interior-first /
    boundaries-after launches of mg_solver.c, and must reproduce its part of the ORACLE's whole-grid result bit for bit."""
    rng = np.random.default_rng(44000 + n + nz + len(cuts))
    nc, nzc = (n - 1) // 2, (nz - 1) // 2
    assert cuts[-1] == nzc
    As = orc.level_stencil(3, n + 2, 0)[0]
    dinv = 1.0 / As[3]
    u, b = rng.uniform(-1, 1, n * n * nz).astype(np.float32), rng.uniform(-1, 1, n * n * nz).astype(np.float32)
    uc = rng.uniform(-1, 1, nc * nc * nzc).astype(np.float32)
    J = lambda x: orc.jacobi32(n, As, SCALE, b, x, nz=nz)
    j1 = J(u)
    j2 = J(j1).reshape(nz, n, n)
    r = orc.residual32(n, As, b, u, nz=nz)
    bc = orc.restrict32(n, r, nzf=nz, nzc=nzc).reshape(nzc, nc, nc)
    pj = J(orc.prolong_add32(n, uc, u, nzf=nz, nzc=nzc)).reshape(nz, n, n)
    j1, r = j1.reshape(nz, n, n), r.reshape(nz, n, n)
    U, B, UC = u.reshape(nz, n, n), b.reshape(nz, n, n), uc.reshape(nzc, nc, nc)
    L, coef = mgk.L, mgk.coef(As)
    for s in range(len(cuts) - 1):
        kc0, kc1 = cuts[s], cuts[s + 1]
        last = s == len(cuts) - 2
        z0, z1 = 2 * kc0, (nz if last else 2 * kc1)
        nzs, nzcs = z1 - z0, kc1 - kc0
        has_lo, has_hi = int(s > 0), int(not last)
        gs, gcs, gfar = _geom32(mgk, n, n, nzs), _geom32(mgk, nc, nc, nzcs), _geom32(mgk, n, n, 2)
        own = []

        def up(pad):
            p = _upload32(mgk, pad)
            own.append(p)
            return p

        def zeros(g):
            f = mgk.field32(g)
            own.append(f)
            return f

        def slab(W):                                        # interior planes and both ghost planes from the whole grid
            return up(_padded32(gs, {k: W[z0 + k] for k in range(-1, nzs + 1) if 0 <= z0 + k < nz}))

        us, bs = slab(U), slab(B)
        far = up(_padded32(gfar, {k: pl for k, pl in ((-1, U[z0 - 2] if has_lo else None), (2, U[z1 + 1] if has_hi else None))
                                  if pl is not None}))
        ucs = up(_padded32(gcs, {k: UC[kc0 + k] for k in range(-1, nzcs + 1) if 0 <= kc0 + k < nzc}))
        tag = f"slab {s} (planes {z0}..{z1 - 1})"

        def check(f, want, g, what):
            got = mgk.from_field32(g, f)
            assert np.array_equal(got, want.ravel()), f"{tag} {what}: {np.count_nonzero(got != want.ravel())} mismatches"
            raw = _raw32(mgk, g, f)
            assert np.count_nonzero(raw) == np.count_nonzero(got), f"{tag} {what}: ghosts written"

        # one sweep and the residual on plane ranges: boundary planes first, then the interior (mg_solver.c, smooth)
        o, rr = zeros(gs), zeros(gs)
        rng_j = ((0, 1), (nzs - 1, nzs), (1, nzs - 1)) if nzs >= 3 else ((0, nzs),)
        for a0, a1 in rng_j:
            mgk._chk(L.mgk_jacobi_range_f32(mgk.ctx, C.byref(gs), coef, dinv, SCALE, bs, us, o, a0, a1, None))
            mgk._chk(L.mgk_residual_range_f32(mgk.ctx, C.byref(gs), coef, bs, us, rr, a0, a1, None))
        check(o, j1[z0:z1], gs, "mgk_jacobi_range_f32")
        check(rr, r[z0:z1], gs, "mgk_residual_range_f32")
        # two sweeps: planes 2 .. nz-3 while the halo travels, then the boundary planes
        o = zeros(gs)
        rng_2 = ((2, nzs - 2), (0, 2), (nzs - 2, nzs)) if nzs >= 6 else ((0, nzs),)
        for a0, a1 in rng_2:
            mgk._chk(L.mgk_jacobi2_slab_f32(mgk.ctx, C.byref(gs), C.byref(gfar), coef, dinv, SCALE, bs, us, o, far, has_lo, has_hi,
                                            a0, a1, None))
        check(o, j2[z0:z1], gs, "mgk_jacobi2_slab_f32")
        # prolongation + sweep: planes 2 .. nz-2 first (no ghost plane of u or uc), then the boundary planes
        o = zeros(gs)
        rng_p = ((2, nzs - 1), (0, 2), (nzs - 1, nzs)) if nzs >= 4 else ((0, nzs),)
        for a0, a1 in rng_p:
            mgk._chk(L.mgk_prolong_jacobi_range_f32(mgk.ctx, C.byref(gs), C.byref(gcs), coef, dinv, SCALE, bs, ucs, us, o, a0, a1, None))
        check(o, pj[z0:z1], gs, "mgk_prolong_jacobi_range_f32")
        # residual + restriction, far-field form: inner coarse planes first, then the two boundary ones
        oc = zeros(gcs)
        rng_c = ((1, nzcs - 1), (0, 1), (nzcs - 1, nzcs)) if nzcs >= 3 else ((0, nzcs),)
        for k0, k1 in rng_c:
            mgk._chk(L.mgk_residual_restrict_slab_f32(mgk.ctx, C.byref(gs), C.byref(gcs), C.byref(gfar), coef, bs, us, far, has_hi, oc,
                                                      k0, k1, None))
        check(oc, bc[kc0:kc1], gcs, "mgk_residual_restrict_slab_f32")
        # ... and the two-exchange form: plane ranges with the last coarse plane left partial, closed by mgk_restrict_finish_f32
        # from the next slab's first residual plane in r's hi ghost plane
        oc = zeros(gcs)
        kmid = nzcs // 2
        rng_r = ((1, kmid), (kmid, nzcs - 1), (0, 1), (nzcs - 1, nzcs)) if nzcs >= 4 else ((0, nzcs),)
        for k0, k1 in rng_r:
            mgk._chk(L.mgk_residual_restrict_range_f32(mgk.ctx, C.byref(gs), C.byref(gcs), coef, bs, us, oc, k0, k1, None))
        if has_hi:
            rv = up(_padded32(gs, {nzs: r[z1]}))
            mgk._chk(L.mgk_restrict_finish_f32(mgk.ctx, C.byref(gs), C.byref(gcs), rv, oc, None))
        check(oc, bc[kc0:kc1], gcs, "mgk_residual_restrict_range_f32 + mgk_restrict_finish_f32")
        for p in own:
            mgk.free(p)


def test_mixed_solve_at_511_equals_the_oracle(orc):
    """BASELINE config 5 at 511^3 (default fuse): the first mixed solve on full-row fp32 levels (511: 2 waves, 255: 1) against
    mgo_vcycle_mixed -- same iteration count, bit-identical solution, residual history to 1e-12"""
    from multigrid_petsc_amd.solver import Solver
    s = Solver(3, 513, 9, v=(3, 3), maxiter=40, scale=SCALE, precision="mixed")
    s.set_rhs_problem()
    it = s.solve()
    rn, u = s.rnorm, s.solution()
    s.close()
    ref = orc.vcycle_mixed(513, 9, maxiter=40, scale=SCALE)
    assert it == ref["iters"], (it, ref["iters"])
    assert np.abs(rn / ref["rnorm"] - 1.0).max() <= 1e-12
    assert np.array_equal(u, ref["u"])


@pytest.mark.timeout(900)
def test_mixed_slab_ranks_at_511_equal_the_oracle(orc):
    """four loopback slab ranks, npts = 513, mixed, default fuse and distribution (levels 511 and 255 on slabs: the fp32 full-row
    kernels with far_lo / far_hi end to end) against mgo_vcycle_mixed, not against the single-rank run"""
    from multigrid_petsc_amd.solver import Solver
    from multigrid_petsc_amd.comm import LoopbackWorld
    P = 4
    world = LoopbackWorld(P)

    def fn(rank, comm):
        s = Solver(3, 513, 9, v=(3, 3), maxiter=40, scale=SCALE, precision="mixed", rank=rank, nranks=P, comm=comm)
        s.set_rhs_problem()
        it = s.solve()
        res = (it, s.rnorm, s.solution())
        s.close()
        return res

    try:
        res = world.run(fn)
    finally:
        world.close()
    ref = orc.vcycle_mixed(513, 9, maxiter=40, scale=SCALE)
    for r in res:
        assert r[0] == ref["iters"], (r[0], ref["iters"])
        assert np.abs(r[1] / ref["rnorm"] - 1.0).max() <= 1e-12
    assert np.array_equal(np.concatenate([r[2] for r in res]), ref["u"])


def _host_mem_gib():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / 2 ** 20
    except OSError:
        pass
    return 0.0


@pytest.mark.timeout(1500)
def test_headline_mixed_cycles_equal_the_oracle_cycles(orc):
    """Config 5 at the headline size (1023^3, 10 levels): two fixed cycles on the GPU against two of mgo_vcycle_mixed; residual
    history to 1e-12, solution bit for bit.  The oracle holds u, b, r in fp64 (3 x 8.6 GB) and u, b, rv, tmp of the fine level in
    fp32 (4 x 4.3 GB, the coarser levels add 1/7), the caller's copy of u (8.6 GB) and the GPU run's solution (8.6 GB): about 65 GB.
    Skipped, with that reason, where the host has less than 90 GiB available."""
    need = 90.0
    have = _host_mem_gib()
    if have < need:
        pytest.skip(f"the oracle's 1023^3 mixed cycle needs ~{need:.0f} GiB of host memory, {have:.0f} GiB available")
    from multigrid_petsc_amd.solver import Solver
    cycles = 2
    s = Solver(3, 1025, 10, v=(3, 3), maxiter=cycles + 1, scale=SCALE, precision="mixed")
    s.set_rhs_problem()
    s.cycles(cycles)
    s.sync()
    rn, u = s.rnorm, s.solution()
    s.close()
    ref = orc.vcycle_mixed(1025, 10, maxiter=cycles, scale=SCALE, fixed_cycles=cycles)
    assert ref["iters"] == cycles and len(rn) == cycles + 1
    assert np.abs(rn / ref["rnorm"] - 1.0).max() <= 1e-12
    assert np.array_equal(u, ref["u"]), "solution after two mixed cycles differs from the oracle's"
