"""3-D grids whose rows are NOT 2^k - 1 wide.  mg_solver_create accepts every npts with npts - 1 divisible by 2^(levels-1) and odd level widths
(97, 193, 385, 641, 769, 897 among them: level widths 95, 191, 383, 639, 767, 895), but every 3-D kernel test runs cubes of 2^k - 1 or thin boxes whose
rows are exactly 128 .. 1024 doubles (the three-sweep kernels excepted): a launcher that calls a row "full" because it is a whole number of waves,
and then runs it in a block of the next built width, is bit-identical on all of them.

One body per shape, on guarded and poisoned buffers (tests/guarded.py), against tests/box_reference.py (numpy; pinned to the oracle by
tests/test_box_reference_cpu.py).  Every 3-D entry point of include/mgk.h / include/mgk_sweep3.h that one rank's cycle calls, fp64 and fp32, is run:
fields are compared bit for bit, sums of squares to RED_RTOL of the reference sum.  u, b, uc and the references are built once per shape and
coefficient set.

Shapes (nx, ny, nz): every nx is 3 mod 4, so the transfer kernels get a coarse partner with an odd nx; the thin extents are (ny, nz) in
{(7, 7), (11, 5), (5, 11)}.  nx + 1 = 12, 24, 48 (short rows), 96 (one partial wave row), 132 (one pair past a wave row), 192 (one and a half), 260 (three
waves needed, run as four, predicated), 384 (three WHOLE waves), 640, 768 (fp32: three whole waves of 256), 896 (five, six, seven whole waves), and
383 once more with (ny + 1) % 4 != 0, where the same width takes the predicated form.  Coefficients: distinct_coef (tests/coef_cases.py; another set
for the coarse level's first sweep) and POW2, six off-diagonals +-2^e, which selects the exact-FMA instances.  Tuning: the default and z chunks of 5;
for mgk_jacobi2_* also the ring / register choice 1 / 2 and the forced forms 36, 37, 39.

Entry points with an _ok_ query: where the query answers 1 the call must succeed and is compared; where it answers 0 the call must refuse.  Which
of the two happened is recorded per entry point (REPORT, printed with -s); every entry point without a query must have compared at least one output
at every shape, every one with a query must have compared or refused at least once, and a shape where nothing at all was compared fails.  The body
collects every mismatch of a shape before it fails, so one run shows all of them.

The slab forms mgk_jacobi2_slab_f64 / _f32 run at 383 and 767 wide with nz = 9 cut at (0, 4, 9); the LDS tails (mgk_tail_cycle_f64 / _f32,
mgk_tail_fmg_f64, mgk_tail_cycle_cheby_f64) at n[0] = 11 (3-D) and 47, 23 (2-D) through the bodies of their own modules."""
import ctypes as C

import numpy as np
import pytest

import box_reference as BR
import test_cheby3_kernels_gpu as CH
import test_distinct_coef_gpu as DC
import test_dropin_kernels_gpu as DK
import test_fmg_gpu as FM
from coef_cases import dense_field, distinct_coef
from guarded import Guarded
from multigrid_petsc_amd.mgk import Geom
from oracle import Oracle

pytestmark = pytest.mark.gpu
RED_RTOL = 1e-13          # the project's figure for sums of squares (tests/test_kernels_gpu.py)
SC, SC_C = 6.0 / 7.0, 0.8
CHEB = (-0.37, 1.37, 0.21)
POW2 = np.array([2.0, -4.0, 1.0, -24.0, -2.0, 8.0, -1.0])          # {k-1, i-1, j-1, C, j+1, i+1, k+1}: the six off-diagonals +-2^e, e >= 0
SHAPES = [(11, 7, 7), (23, 11, 5), (47, 5, 11), (95, 7, 7), (131, 11, 5), (191, 5, 11), (259, 7, 7), (383, 11, 5), (383, 5, 11), (639, 7, 7),
          (767, 11, 5), (895, 7, 7)]                                 # (nx, ny, nz)
BASE = ((-1, -1), (-1, 5))
J2 = BASE + ((1, -1), (2, -1), (36, -1), (37, -1), (39, -1))
REPORT = {}               # (nx, ny, nz) -> {entry point: [outputs compared, calls refused after _ok_ == 0]}


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _geom32(G, nx, ny, nz):
    g = Geom()
    G._chk(G.L.mgk_geom_init_f32(C.byref(g), 3, nx, ny, nz))
    return g


class Box:
    """one shape: the device inputs, the references of one coefficient set, and the comparison of one call's outputs"""

    def __init__(self, G, orc, nx, ny, nz):
        self.G, self.orc, self.L, self.shape = G, orc, G.L, (nx, ny, nz)
        rng = np.random.default_rng([96000, nx, ny, nz])
        self.nzc, self.nyc, self.nxc = BR.coarse_shape(nz, ny, nx)
        self.gf, self.gc = G.geom(3, nx, ny, nz), G.geom(3, self.nxc, self.nyc, self.nzc)
        self.gf32, self.gc32 = _geom32(G, nx, ny, nz), _geom32(G, self.nxc, self.nyc, self.nzc)
        self.u, self.b, self.pm = (dense_field(rng, nz, ny, nx) for _ in range(3))
        self.uc = dense_field(rng, self.nzc, self.nyc, self.nxc)
        self.e32 = dense_field(rng, nz, ny, nx).astype(np.float32)
        self.u32, self.b32, self.uc32 = (a.astype(np.float32) for a in (self.u, self.b, self.uc))
        self.As, self.Ac = distinct_coef(rng, 3, per_level=2)
        self.du, self.db, self.dpm, self.duc = (G.to_field(g, a) for g, a in ((self.gf, self.u), (self.gf, self.b), (self.gf, self.pm), (self.gc, self.uc)))
        self.du32, self.db32, self.de32 = (G.to_field32(self.gf32, a) for a in (self.u32, self.b32, self.e32))
        self.duc32 = G.to_field32(self.gc32, self.uc32)
        self.own = [self.du, self.db, self.dpm, self.duc, self.du32, self.db32, self.de32, self.duc32]
        self.ss = C.c_double()
        self.took = REPORT.setdefault(self.shape, {})
        self.failures = []

    # ---- references ----
    def refs(self, As, u, b, uc, pm=None):
        """everything the calls are compared with for the operator As, in the precision of the fields handed in"""
        J = lambda x: BR.sweep(As, SC, b, x)
        r = {}
        r["j1"] = J(u)
        r["j2"] = J(r["j1"])
        r["j3"] = J(r["j2"])
        r["z1"] = BR.sweep_zero(As, SC, b)
        r["z3"] = J(J(r["z1"]))
        r["r0"] = BR.residual(As, b, u)
        r["r1"] = BR.residual(As, b, r["j1"])
        r["au"] = BR.apply(As, u)
        r["rfw"] = BR.restrict(u)
        r["bc0"], r["bc1"] = BR.restrict(r["r0"]), BR.restrict(r["r1"])
        r["uc0_0"], r["uc0_1"] = BR.sweep_zero(self.Ac, SC_C, r["bc0"]), BR.sweep_zero(self.Ac, SC_C, r["bc1"])
        r["pu"] = BR.prolong_add(uc, u)
        r["pj1"] = J(r["pu"])
        r["pj2"] = J(r["pj1"])
        r["pj3"] = J(r["pj2"])
        r["i2"] = J(J(BR.prolong_add(uc, np.zeros_like(u))))
        if pm is not None:
            r["ch"] = BR.cheby_step(As, b, u, pm, *CHEB)
        if u.dtype == np.float64:
            sq = lambda a: self.orc.sumsq(np.ascontiguousarray(a).ravel())
            r["ss0"], r["ss1"], r["ssu"] = sq(r["r0"]), sq(r["r1"]), sq(u)
            # the fp64 <-> fp32 bridges of the mixed-precision outer step
            r["r0_32"] = r["r0"].astype(np.float32)
            r["e0_0"] = BR.sweep_zero(As, SC, r["r0_32"])
            r["ucorr"] = u + self.e32.astype(np.float64)
            rc = BR.residual(As, b, r["ucorr"])
            r["rc_32"], r["ssc"] = rc.astype(np.float32), sq(rc)
            r["e0_c"] = BR.sweep_zero(As, SC, r["rc_32"])
        return r

    # ---- outputs ----
    def out(self, coarse=False, f32=False):
        g = (self.gc32 if coarse else self.gf32) if f32 else (self.gc if coarse else self.gf)
        return (self.G.field32 if f32 else self.G.field)(g), g, f32

    def _note(self, name, compared=0, refused=0):
        e = self.took.setdefault(name, [0, 0])
        e[0] += compared
        e[1] += refused

    def call(self, name, tag, fn, outs, sumsq=None, ok=None):
        """fn(): the return code.  outs: [((device field, geometry, is it fp32), reference)]; every output is freed here.  ok: the answer of the entry
        point's _ok_ query (None: it has none): 0 -> the call must refuse and nothing is compared.  Mismatches are collected, not raised"""
        G = self.G
        what = f"{name} {self.shape} {tag}"
        if sumsq is not None:
            self.ss.value = np.nan                   # a call that leaves its sum unwritten must not find the one before
        try:
            rc = fn()
            if ok is not None and not ok:
                if rc == 0:
                    self.failures.append(f"{what}: the _ok_ query answered 0 and the call did not refuse")
                else:
                    self._note(name, refused=1)
                return
            if rc != 0:
                self.failures.append(f"{what}: rc={rc}: {G.last_error()}" + (" although the _ok_ query answered 1" if ok else ""))
                return
            for (f, g, f32), want in outs:
                got = (G.from_field32 if f32 else G.from_field)(g, f).reshape(want.shape)          # guards and frame
                assert got.dtype == want.dtype
                bad = np.argwhere(got != want)
                if bad.size:
                    self.failures.append(f"{what}: {len(bad)} of {want.size} cells differ ({np.count_nonzero(np.isnan(got))} NaN), the first (k, i, j): "
                                         f"{bad[:4].tolist()}, the last: {bad[-1].tolist()}")
                else:
                    self._note(name, compared=1)
            if sumsq is not None:
                if not abs(self.ss.value - sumsq) <= RED_RTOL * sumsq:
                    self.failures.append(f"{what}: sum of squares {self.ss.value!r} vs {sumsq!r}")
                else:
                    self._note(name, compared=1)
        except AssertionError as e:                    # a guard zone or the frame
            self.failures.append(f"{what}: {e}")
        finally:
            for (f, _, _), _ in outs:
                try:
                    G.free(f)
                except AssertionError as e:
                    self.failures.append(f"{what}: at free: {e}")
                    G.inner.free(G.live.pop(G._addr(f)).base)

    def untouched(self):
        G = self.G
        for g, f, a in ((self.gf, self.du, self.u), (self.gf, self.db, self.b), (self.gf, self.dpm, self.pm), (self.gc, self.duc, self.uc)):
            assert np.array_equal(G.from_field(g, f), a.ravel()), "an input field was modified"
        for g, f, a in ((self.gf32, self.du32, self.u32), (self.gf32, self.db32, self.b32), (self.gf32, self.de32, self.e32), (self.gc32, self.duc32, self.uc32)):
            assert np.array_equal(G.from_field32(g, f), a.ravel()), "an fp32 input field was modified"

    def close(self):
        for p in self.own:
            self.G.free(p)


def _tune(L, var, zc):
    L.mgk_set_tuning(var, zc)
    return f"variant={var} zc={zc}"


def _ranges(n):
    """the plane ranges of a slab rank: the inner planes first, then the two boundary planes"""
    return ((1, n - 1), (0, 1), (n - 1, n)) if n >= 3 else ((0, n),)


def _fp64(t, As, cname):
    G, L, ctx, ss = t.G, t.L, t.G.ctx, C.byref(t.ss)
    g, gc, g32, du, db, dpm, duc, de32 = C.byref(t.gf), C.byref(t.gc), C.byref(t.gf32), t.du, t.db, t.dpm, t.duc, t.de32
    coef, dinv, dinv_c = G.coef(As), 1.0 / As[3], 1.0 / t.Ac[3]
    r = t.refs(As, t.u, t.b, t.uc, t.pm)
    nz, nzc = t.shape[2], t.nzc
    O = t.out
    for var, zc in BASE:
        tag = f"{cname} {_tune(L, var, zc)}"
        o = O()
        t.call("mgk_jacobi_f64", tag, lambda: L.mgk_jacobi_f64(ctx, g, coef, dinv, SC, db, du, o[0], None), [(o, r["j1"])])
        o = O()

        def ranged(fn):
            for z0, z1 in _ranges(nz):
                rc = fn(z0, z1)
                if rc:
                    return rc
            return 0
        t.call("mgk_jacobi_range_f64", tag, lambda: ranged(lambda z0, z1: L.mgk_jacobi_range_f64(ctx, g, coef, dinv, SC, db, du, o[0], z0, z1, None)), [(o, r["j1"])])
        o = O()
        t.call("mgk_jacobi_zero_f64", tag, lambda: L.mgk_jacobi_zero_f64(ctx, g, dinv, SC, db, o[0], None), [(o, r["z1"])])
        o = O()
        t.call("mgk_cheby_f64", tag, lambda: L.mgk_cheby_f64(ctx, g, coef, dinv, *CHEB, db, du, dpm, o[0], None), [(o, r["ch"])])
        o = O()
        t.call("mgk_residual_f64", tag, lambda: L.mgk_residual_f64(ctx, g, coef, db, du, o[0], None), [(o, r["r0"])])
        o = O()
        t.call("mgk_residual_range_f64", tag, lambda: ranged(lambda z0, z1: L.mgk_residual_range_f64(ctx, g, coef, db, du, o[0], z0, z1, None)), [(o, r["r0"])])
        o = O()
        t.call("mgk_apply_f64", tag, lambda: L.mgk_apply_f64(ctx, g, coef, du, o[0], None), [(o, r["au"])])
        t.call("mgk_sumsq_f64", tag, lambda: L.mgk_sumsq_f64(ctx, g, du, ss, None), [], r["ssu"])
        t.call("mgk_residual_sumsq_f64", tag, lambda: L.mgk_residual_sumsq_f64(ctx, g, coef, db, du, ss, None), [], r["ss0"])
        o = O()
        t.call("mgk_jacobi_sumsq_f64", tag, lambda: L.mgk_jacobi_sumsq_f64(ctx, g, coef, dinv, SC, db, du, o[0], ss, None), [(o, r["j1"])], r["ss0"])
        o = O()

        def sumsq_ranges():
            off, npart = 0, C.c_int()
            for z0, z1 in _ranges(nz):
                rc = L.mgk_jacobi_sumsq_range_f64(ctx, g, coef, dinv, SC, db, du, o[0], z0, z1, off, C.byref(npart), None)
                if rc:
                    return rc
                off += npart.value
            return L.mgk_partials_finish(ctx, off, ss, None)
        t.call("mgk_jacobi_sumsq_range_f64", tag, sumsq_ranges, [(o, r["j1"])], r["ss0"])
        # three sweeps per pass (mgk_sweep3.hip): any shape; the stacked norm / prolongation forms where their queries offer them
        o = O()
        t.call("mgk_jacobi3_f64", tag, lambda: L.mgk_jacobi3_f64(ctx, g, coef, dinv, SC, db, du, o[0], None), [(o, r["j3"])])
        o = O()
        t.call("mgk_jacobi3_sumsq_f64", tag, lambda: L.mgk_jacobi3_sumsq_f64(ctx, g, coef, dinv, SC, db, du, o[0], ss, None), [(o, r["j3"])], r["ss0"])
        o = O()
        t.call("mgk_jacobi3_sumsq_mid_f64", tag, lambda: L.mgk_jacobi3_sumsq_mid_f64(ctx, g, coef, dinv, SC, db, du, o[0], ss, None), [(o, r["j3"])], r["ss1"],
               ok=L.mgk_jacobi3_mid_ok_f64(g))
        o = O()
        t.call("mgk_prolong_jacobi3_f64", tag, lambda: L.mgk_prolong_jacobi3_f64(ctx, g, gc, coef, dinv, SC, db, duc, du, o[0], None), [(o, r["pj3"])],
               ok=L.mgk_prolong_jacobi3_ok_f64(g, gc))
        # transfers and the passes fused with them
        o = O(1)
        t.call("mgk_restrict_fw_f64", tag, lambda: L.mgk_restrict_fw_f64(ctx, g, gc, du, o[0], None), [(o, r["rfw"])])
        o = (G.to_field(t.gf, t.u), t.gf, False)                    # in place: on a copy of u
        t.call("mgk_prolong_add_f64", tag, lambda: L.mgk_prolong_add_f64(ctx, g, gc, duc, o[0], None), [(o, r["pu"])])
        o = O(1)
        t.call("mgk_residual_restrict_f64", tag, lambda: L.mgk_residual_restrict_f64(ctx, g, gc, coef, db, du, o[0], None), [(o, r["bc0"])])
        o = O(1)

        def rr_ranges():
            for k0, k1 in _ranges(nzc):
                rc = L.mgk_residual_restrict_range_f64(ctx, g, gc, coef, db, du, o[0], k0, k1, None)
                if rc:
                    return rc
            return 0
        t.call("mgk_residual_restrict_range_f64", tag, rr_ranges, [(o, r["bc0"])])
        o, o2 = O(1), O(1)
        t.call("mgk_residual_restrict_jz_f64", tag, lambda: L.mgk_residual_restrict_jz_f64(ctx, g, gc, coef, db, du, o[0], o2[0], dinv_c, SC_C, None),
               [(o, r["bc0"]), (o2, r["uc0_0"])])
        o = O()
        t.call("mgk_prolong_jacobi_f64", tag, lambda: L.mgk_prolong_jacobi_f64(ctx, g, gc, coef, dinv, SC, db, duc, du, o[0], None), [(o, r["pj1"])])
        o = O()
        t.call("mgk_prolong_jacobi_range_f64", tag,
               lambda: ranged(lambda z0, z1: L.mgk_prolong_jacobi_range_f64(ctx, g, gc, coef, dinv, SC, db, duc, du, o[0], z0, z1, None)), [(o, r["pj1"])])
        o = O()
        t.call("mgk_prolong_jacobi2_f64", tag, lambda: L.mgk_prolong_jacobi2_f64(ctx, g, gc, coef, dinv, SC, db, duc, du, o[0], None), [(o, r["pj2"])],
               ok=L.mgk_prolong_jacobi2_ok_f64(g, gc))
        o = O()
        t.call("mgk_interp_jacobi2_f64", tag, lambda: L.mgk_interp_jacobi2_f64(ctx, g, gc, coef, dinv, SC, db, duc, o[0], None), [(o, r["i2"])],
               ok=L.mgk_interp_jacobi2_ok_f64(g, gc))
        ok = L.mgk_sweep_residual_restrict_ok_f64(g, gc)
        o, o2, o3 = O(), O(1), O(1)
        t.call("mgk_sweep_residual_restrict_f64", tag,
               lambda: L.mgk_sweep_residual_restrict_f64(ctx, g, gc, coef, dinv, SC, db, du, o[0], o2[0], o3[0], dinv_c, SC_C, None),
               [(o, r["j1"]), (o2, r["bc1"]), (o3, r["uc0_1"])], ok=ok)
        o, o2 = O(), O(1)
        t.call("mgk_sweep_residual_restrict_f64", tag + " uc0=NULL",
               lambda: L.mgk_sweep_residual_restrict_f64(ctx, g, gc, coef, dinv, SC, db, du, o[0], o2[0], None, dinv_c, SC_C, None),
               [(o, r["j1"]), (o2, r["bc1"])], ok=ok)
        # the bridges of the mixed-precision outer step
        o = O(f32=True)
        t.call("mgk_residual_f64_to_f32", tag, lambda: L.mgk_residual_f64_to_f32(ctx, g, g32, coef, db, du, o[0], ss, None), [(o, r["r0_32"])], r["ss0"])
        o, o2 = O(f32=True), O(f32=True)
        t.call("mgk_residual_f64_to_f32_jz", tag, lambda: L.mgk_residual_f64_to_f32_jz(ctx, g, g32, coef, db, du, o[0], o2[0], dinv, SC, ss, None),
               [(o, r["r0_32"]), (o2, r["e0_0"])], r["ss0"])
        o, o2 = O(), O(f32=True)
        t.call("mgk_correct_residual_f64_f32", tag, lambda: L.mgk_correct_residual_f64_f32(ctx, g, g32, coef, db, du, de32, o[0], o2[0], ss, None),
               [(o, r["ucorr"]), (o2, r["rc_32"])], r["ssc"])
        o, o2, o3 = O(), O(f32=True), O(f32=True)
        t.call("mgk_correct_residual_f64_f32_jz", tag,
               lambda: L.mgk_correct_residual_f64_f32_jz(ctx, g, g32, coef, db, du, de32, o[0], o2[0], o3[0], dinv, SC, ss, None),
               [(o, r["ucorr"]), (o2, r["rc_32"]), (o3, r["e0_c"])], r["ssc"])
        o = (G.to_field(t.gf, t.u), t.gf, False)
        t.call("mgk_correct_f64_from_f32", tag, lambda: L.mgk_correct_f64_from_f32(ctx, g, g32, de32, o[0], None), [(o, r["ucorr"])])
    for var, zc in J2:
        tag = f"{cname} {_tune(L, var, zc)}"                        # (the queries read the tuning variant: they are asked under it)
        o = O()
        t.call("mgk_jacobi2_f64", tag, lambda: L.mgk_jacobi2_f64(ctx, g, coef, dinv, SC, db, du, o[0], None), [(o, r["j2"])])
        o = O()
        t.call("mgk_jacobi2_zero_f64", tag, lambda: L.mgk_jacobi2_zero_f64(ctx, g, coef, dinv, SC, db, o[0], None), [(o, r["z3"])],
               ok=L.mgk_jacobi2_zero_ok_f64(g))
        ok = L.mgk_jacobi2_sumsq_ok_f64(g)
        o = O()
        t.call("mgk_jacobi2_sumsq_f64", tag, lambda: L.mgk_jacobi2_sumsq_f64(ctx, g, coef, dinv, SC, db, du, o[0], ss, None), [(o, r["j2"])], r["ss0"], ok=ok)
        o = O()
        t.call("mgk_jacobi2_sumsq_mid_f64", tag, lambda: L.mgk_jacobi2_sumsq_mid_f64(ctx, g, coef, dinv, SC, db, du, o[0], ss, None), [(o, r["j2"])], r["ss1"],
               ok=ok)
    L.mgk_set_tuning(-1, -1)


def _fp32(t, As, cname):
    G, L, ctx = t.G, t.L, t.G.ctx
    g, gc, du, db, duc = C.byref(t.gf32), C.byref(t.gc32), t.du32, t.db32, t.duc32
    coef, dinv, dinv_c = G.coef(As), 1.0 / As[3], 1.0 / t.Ac[3]
    r = t.refs(As, t.u32, t.b32, t.uc32)
    assert all(v.dtype == np.float32 for v in r.values())
    nz, nzc = t.shape[2], t.nzc
    O = lambda coarse=False: t.out(coarse, f32=True)

    def ranged(fn, n=nz):
        for z0, z1 in _ranges(n):
            rc = fn(z0, z1)
            if rc:
                return rc
        return 0
    for var, zc in BASE:
        tag = f"{cname} {_tune(L, var, zc)}"
        o = O()
        t.call("mgk_jacobi_f32", tag, lambda: L.mgk_jacobi_f32(ctx, g, coef, dinv, SC, db, du, o[0], None), [(o, r["j1"])])
        o = O()
        t.call("mgk_jacobi_range_f32", tag, lambda: ranged(lambda z0, z1: L.mgk_jacobi_range_f32(ctx, g, coef, dinv, SC, db, du, o[0], z0, z1, None)), [(o, r["j1"])])
        o = O()
        t.call("mgk_jacobi_zero_f32", tag, lambda: L.mgk_jacobi_zero_f32(ctx, g, dinv, SC, db, o[0], None), [(o, r["z1"])])
        o = O()
        t.call("mgk_residual_f32", tag, lambda: L.mgk_residual_f32(ctx, g, coef, db, du, o[0], None), [(o, r["r0"])])
        o = O()
        t.call("mgk_residual_range_f32", tag, lambda: ranged(lambda z0, z1: L.mgk_residual_range_f32(ctx, g, coef, db, du, o[0], z0, z1, None)), [(o, r["r0"])])
        o = O(1)
        t.call("mgk_restrict_fw_f32", tag, lambda: L.mgk_restrict_fw_f32(ctx, g, gc, du, o[0], None), [(o, r["rfw"])])
        o = (G.to_field32(t.gf32, t.u32), t.gf32, True)
        t.call("mgk_prolong_add_f32", tag, lambda: L.mgk_prolong_add_f32(ctx, g, gc, duc, o[0], None), [(o, r["pu"])])
        o = O(1)
        t.call("mgk_residual_restrict_f32", tag, lambda: L.mgk_residual_restrict_f32(ctx, g, gc, coef, db, du, o[0], None), [(o, r["bc0"])])
        o = O(1)
        t.call("mgk_residual_restrict_range_f32", tag,
               lambda: ranged(lambda k0, k1: L.mgk_residual_restrict_range_f32(ctx, g, gc, coef, db, du, o[0], k0, k1, None), nzc), [(o, r["bc0"])])
        o, o2 = O(1), O(1)
        t.call("mgk_residual_restrict_jz_f32", tag, lambda: L.mgk_residual_restrict_jz_f32(ctx, g, gc, coef, db, du, o[0], o2[0], dinv_c, SC_C, None),
               [(o, r["bc0"]), (o2, r["uc0_0"])])
        o = O()
        t.call("mgk_prolong_jacobi_f32", tag, lambda: L.mgk_prolong_jacobi_f32(ctx, g, gc, coef, dinv, SC, db, duc, du, o[0], None), [(o, r["pj1"])])
        o = O()
        t.call("mgk_prolong_jacobi_range_f32", tag,
               lambda: ranged(lambda z0, z1: L.mgk_prolong_jacobi_range_f32(ctx, g, gc, coef, dinv, SC, db, duc, du, o[0], z0, z1, None)), [(o, r["pj1"])])
    for var, zc in J2:
        tag = f"{cname} {_tune(L, var, zc)}"
        o = O()
        t.call("mgk_jacobi2_f32", tag, lambda: L.mgk_jacobi2_f32(ctx, g, coef, dinv, SC, db, du, o[0], None), [(o, r["j2"])])
        o = O()
        t.call("mgk_jacobi2_zero_f32", tag, lambda: L.mgk_jacobi2_zero_f32(ctx, g, coef, dinv, SC, db, o[0], None), [(o, r["z3"])],
               ok=L.mgk_jacobi2_zero_ok_f32(g))
    L.mgk_set_tuning(-1, -1)


GATED = ("mgk_jacobi3_sumsq_mid_f64 mgk_prolong_jacobi3_f64 mgk_prolong_jacobi2_f64 mgk_interp_jacobi2_f64 mgk_sweep_residual_restrict_f64 "
         "mgk_jacobi2_zero_f64 mgk_jacobi2_sumsq_f64 mgk_jacobi2_sumsq_mid_f64 mgk_jacobi2_zero_f32").split()
UNGATED = ("mgk_jacobi_f64 mgk_jacobi_range_f64 mgk_jacobi_zero_f64 mgk_cheby_f64 mgk_residual_f64 mgk_residual_range_f64 mgk_apply_f64 mgk_sumsq_f64 "
           "mgk_residual_sumsq_f64 mgk_jacobi_sumsq_f64 mgk_jacobi_sumsq_range_f64 mgk_jacobi3_f64 mgk_jacobi3_sumsq_f64 mgk_restrict_fw_f64 "
           "mgk_prolong_add_f64 mgk_residual_restrict_f64 mgk_residual_restrict_range_f64 mgk_residual_restrict_jz_f64 mgk_prolong_jacobi_f64 "
           "mgk_prolong_jacobi_range_f64 mgk_residual_f64_to_f32 mgk_residual_f64_to_f32_jz mgk_correct_residual_f64_f32 mgk_correct_residual_f64_f32_jz "
           "mgk_correct_f64_from_f32 mgk_jacobi2_f64 mgk_jacobi_f32 mgk_jacobi_range_f32 mgk_jacobi_zero_f32 mgk_residual_f32 mgk_residual_range_f32 "
           "mgk_restrict_fw_f32 mgk_prolong_add_f32 mgk_residual_restrict_f32 mgk_residual_restrict_range_f32 mgk_residual_restrict_jz_f32 "
           "mgk_prolong_jacobi_f32 mgk_prolong_jacobi_range_f32 mgk_jacobi2_f32").split()


@pytest.mark.parametrize("nx,ny,nz", SHAPES)
def test_every_3d_entry_point_on_an_off_width_box(mgk, orc, nx, ny, nz):
    G = Guarded(mgk)
    try:
        t = Box(G, orc, nx, ny, nz)
        for cname, As in (("distinct", t.As), ("pow2", POW2)):
            _fp64(t, As, cname)
            _fp32(t, As, cname)
        print(f"\n{(nx, ny, nz)}: " + ", ".join(f"{k} {'compared ' + str(v[0]) if v[0] else ''}{' refused ' + str(v[1]) if v[1] else ''}" for k, v in sorted(t.took.items())))
        assert not t.failures, f"{len(t.failures)} mismatches at {(nx, ny, nz)}:\n" + "\n".join(t.failures[:60])
        empty = [k for k in UNGATED if not t.took.get(k, [0, 0])[0]]
        assert not empty, f"nothing was compared for {empty}"
        empty = [k for k in GATED if not sum(t.took.get(k, [0, 0]))]
        assert not empty, f"neither compared nor refused: {empty}"
        assert set(t.took) == set(GATED) | set(UNGATED), sorted(set(t.took) ^ (set(GATED) | set(UNGATED)))
        t.untouched()
        t.close()
        G.assert_no_leaks()
        assert G.frame_checks > 100
    finally:
        G.release()
        mgk.L.mgk_set_tuning(-1, -1)


def test_the_whole_row_forms_are_taken_at_1_2_4_8_waves_only(mgk):
    """the queries at the listed widths: rows of 3, 5, 6, 7 whole waves are not offered the full-row forms (they would run in a block one size up)"""
    L = mgk.L
    for nx in (383, 639, 767, 895, 259, 95):
        g, gc = mgk.geom(3, nx, 7, 7), mgk.geom(3, (nx - 1) // 2, 3, 3)
        for q in (L.mgk_jacobi2_sumsq_ok_f64, L.mgk_jacobi2_zero_ok_f64):
            assert q(C.byref(g)) == 0, (nx, q)
        for q in (L.mgk_sweep_residual_restrict_ok_f64, L.mgk_prolong_jacobi2_ok_f64, L.mgk_interp_jacobi2_ok_f64):
            assert q(C.byref(g), C.byref(gc)) == 0, (nx, q)
    for nx in (127, 255, 511, 1023):
        g = mgk.geom(3, nx, 7, 7)
        assert L.mgk_jacobi2_sumsq_ok_f64(C.byref(g)) == 1 and L.mgk_jacobi2_zero_ok_f64(C.byref(g)) == 1, nx
    for nx, want in ((767, 0), (383, 0), (255, 1), (511, 1), (1023, 1)):
        g32 = Geom()
        mgk._chk(L.mgk_geom_init_f32(C.byref(g32), 3, nx, 7, 7))
        assert L.mgk_jacobi2_zero_ok_f32(C.byref(g32)) == want, nx


@pytest.mark.parametrize("nx,prec", [(383, "f64"), (767, "f64"), (383, "f32"), (767, "f32")])
def test_two_sweeps_on_z_slabs_of_an_off_width_box(mgk, nx, prec):
    """mgk_jacobi2_slab_f64 / _f32 on the slabs (0, 4, 9) of an nx x 7 x 9 box: every slab, given its neighbours' planes the way the halo exchange
    delivers them (ghost planes of u and b; far: lo = plane z0 - 2, hi = plane z1 + 1 of u), reproduces the two sweeps on its planes"""
    ny, nz, cuts = 7, 9, (0, 4, 9)
    f32 = prec == "f32"
    dt = np.float32 if f32 else np.float64
    rng = np.random.default_rng(96500 + nx)
    G = Guarded(mgk)
    L = G.L
    try:
        for cname, As in (("distinct", distinct_coef(rng, 3)), ("pow2", POW2)):
            U, B = dense_field(rng, nz, ny, nx).astype(dt), dense_field(rng, nz, ny, nx).astype(dt)
            want = BR.sweep(As, SC, B, BR.sweep(As, SC, B, U))
            geom = (lambda k: _geom32(G, nx, ny, k)) if f32 else (lambda k: G.geom(3, nx, ny, k))

            def image(g, planes):
                """a padded image of geometry g: planes = {k (-1 .. g.nz): (ny, nx) array}"""
                raw = np.zeros(g.total, dtype=dt)
                for k, pl in planes.items():
                    for i in range(ny):
                        o = g.org + k * g.plane + i * g.pitch
                        raw[o:o + nx] = pl[i]
                return G._new(raw.nbytes, raw, init=raw.copy())
            for var, zc in BASE + ((36, -1), (37, -1)):
                L.mgk_set_tuning(var, zc)
                for s in range(len(cuts) - 1):
                    z0, z1 = cuts[s], cuts[s + 1]
                    n, has_lo, has_hi = z1 - z0, int(z0 > 0), int(z1 < nz)
                    gs, gfar = geom(n), geom(2)
                    us = image(gs, {k: U[z0 + k] for k in range(-1, n + 1) if 0 <= z0 + k < nz})
                    bs = image(gs, {k: B[z0 + k] for k in range(-1, n + 1) if 0 <= z0 + k < nz})
                    far = image(gfar, {k: U[z] for k, z, has in ((-1, z0 - 2, has_lo), (2, z1 + 1, has_hi)) if has and 0 <= z < nz})
                    out = (G.field32 if f32 else G.field)(gs)
                    fn = L.mgk_jacobi2_slab_f32 if f32 else L.mgk_jacobi2_slab_f64
                    for a0, a1 in ((1, n - 1), (0, 1), (n - 1, n)):
                        G._chk(fn(G.ctx, C.byref(gs), C.byref(gfar), G.coef(As), 1.0 / As[3], SC, bs, us, out, far, has_lo, has_hi, a0, a1, None))
                    got = (G.from_field32 if f32 else G.from_field)(gs, out).reshape(n, ny, nx)
                    bad = np.argwhere(got != want[z0:z1])
                    assert bad.size == 0, f"{cname} variant={var} zc={zc} slab {s}: {len(bad)} cells differ, the first (k, i, j): {bad[:4].tolist()}"
                    for p in (us, bs, far, out):
                        G.free(p)
        G.assert_no_leaks()
    finally:
        G.release()
        mgk.L.mgk_set_tuning(-1, -1)


TAILS = [(DC.test_tail_cycle_with_a_set_per_level, (3, 11, 2, 3, 3)), (DC.test_tail_cycle_with_a_set_per_level, (2, 47, 4, 3, 3)),
         (DC.test_tail_cycle_with_a_set_per_level, (2, 23, 3, 2, 1)),
         (DK.test_tail_cycle_f32_bit_exact, (11, 2, 3, 3)),
         (FM.test_tail_fmg_equals_the_restatement, (3, 11, 2, 1)), (FM.test_tail_fmg_equals_the_restatement, (2, 47, 4, 2)),
         (FM.test_tail_fmg_equals_the_restatement, (2, 23, 3, 1)),
         (CH.test_cheby_tail_kernel_bit_exact, (3, 11, 2, (2, 1))), (CH.test_cheby_tail_kernel_bit_exact, (2, 47, 4, (3, 3))),
         (CH.test_cheby_tail_kernel_bit_exact, (2, 23, 3, (3, 3)))]


@pytest.mark.parametrize("body,args", TAILS, ids=[f"{b.__name__[5:]}-{'-'.join(map(str, a))}".replace(" ", "") for b, a in TAILS])
def test_lds_tails_at_off_widths(mgk, orc, body, args):
    """the tail kernels against the kernel-per-operation walk of their own modules, at first-level widths 11, 47 and 23, on guarded buffers"""
    G = Guarded(mgk)
    try:
        body(G, orc, *args)
        G.assert_no_leaks()
        assert G.frame_checks + G.whole_downloads >= 1
    finally:
        G.release()
        mgk.L.mgk_set_tuning(-1, -1)
