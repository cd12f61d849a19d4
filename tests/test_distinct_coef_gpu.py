"""Every coefficient-taking entry point of the kernel ABI (include/mgk.h) on NON-SYMMETRIC coefficients (tests/coef_cases.py): seven
(2-D: five) pairwise distinct values of mixed sign, row tables with W != E, another set on every level.  The level stencils the other
GPU modules use have equal off-diagonal entries; a kernel that reads one slot for another, a host-side loader that transposes two,
or a tail kernel that takes another level's constants gives the same bits there and an O(1) difference here.

Rules of the suite: fields bit for bit against the CPU oracle composed operation by operation (orc.jacobi / residual / cheby_step /
restrict / prolong_add, the *32 forms for fp32, tests/row_tables.py for the row tables; tests/test_distinct_coef_cpu.py pins the
oracle itself to numpy on such coefficients); reductions to RED_RTOL of orc.sumsq; no GPU result is compared with another GPU result;
ghosts and padding stay zero, inputs stay untouched.  Inputs are dense (no exact zero).

Two kinds of cases:
 * REUSED: test bodies of the other GPU modules that take their coefficients from orc.level_stencil(...) and compare with nothing but
   the oracle, handed a DistinctOracle -- the same calls, tuning variants and assertions, on the smallest shapes that still reach the
   form under test (full-row 3-D forms: thin grids 511 / 1023 wide).
 * bodies written here, for the entry points whose own tests build [q, q, -4q, q, q] themselves or compare with a sibling kernel.
   Scale 6/7 on the fine level, 0.8 with the coarse level's own constants where a pass also starts the coarse level.

tests/test_distinct_coef_cpu.py fails when an entry point with a coef / coef7 / ctab / ctab_f / dtab parameter is not named below."""
import ctypes as C

import numpy as np
import pytest

import test_dropin_kernels_gpu as DK
import test_fmg_gpu as FM
import test_headline_width_gpu as HW
import test_kernels_gpu as K
import test_mixed_gpu as MX
import test_mixed_width_gpu as MW
from cheby_reference import cheb7, ksp_solve, ksp_solve_rt
from coef_cases import DistinctOracle, dense_field, distinct_coef, distinct_row_tables
from row_tables import _rt_apply, _rt_jacobi

pytestmark = pytest.mark.gpu
RED_RTOL = 1e-13          # the project's figure for sums of squares (tests/test_kernels_gpu.py)
SC, SC_C = 6.0 / 7.0, 0.8
CHEB = (-0.37, 1.37, 0.21)
EIG = (0.5, 2.0)          # omega > 1 in the steps 2 and 3


@pytest.fixture(scope="module")
def orc():
    return DistinctOracle()


@pytest.fixture(autouse=True)
def _default_tuning(mgk):
    yield
    mgk.L.mgk_set_tuning(-1, -1)


class Dev:
    """device buffers of one test, freed together"""

    def __init__(self, mgk):
        self.mgk, self.own = mgk, []

    def keep(self, p):
        self.own.append(p)
        return p

    def field(self, g, data=None):
        return self.keep(self.mgk.field(g) if data is None else self.mgk.to_field(g, np.ascontiguousarray(data).ravel()))

    def up(self, arr):
        return self.keep(self.mgk.upload(np.ascontiguousarray(arr).ravel()))

    def zero(self, g, *fields):
        for f in fields:
            self.mgk._chk(self.mgk.L.mgk_memset0(self.mgk.ctx, f, 8 * g.total, None))

    def close(self):
        for p in self.own:
            self.mgk.free(p)


def _same(mgk, g, f, want, what):
    """the field equals `want` bit for bit and nothing but the interior of its allocation was written"""
    got = mgk.from_field(g, f)
    want = np.ascontiguousarray(want).ravel()
    assert np.array_equal(got, want), f"{what}: {np.count_nonzero(got != want)} of {want.size} differ, max {np.abs(got - want).max()}"
    assert np.count_nonzero(mgk.raw_field(g, f)) == np.count_nonzero(got), f"{what}: a ghost or padding cell was written"


def _red(orc, ss, r, what):
    ref = orc.sumsq(np.ascontiguousarray(r).ravel())
    assert abs(ss.value - ref) <= RED_RTOL * ref, f"{what}: {ss.value} vs {ref}"


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ------------------------------------------------------------------------------------------------------------------------------
# REUSED bodies.  (body, arguments after (mgk, orc), the entry points it runs)
# ------------------------------------------------------------------------------------------------------------------------------
REUSED = [
    # A. single pass
    (K.test_stencil_modes_bit_exact, (3, 7, 2), "mgk_jacobi_f64 mgk_residual_f64 mgk_residual_sumsq_f64 mgk_cheby_f64"),
    (K.test_stencil_modes_bit_exact, (3, 127, 34), "... the row form of the sweep (k_jrow) forced"),
    (K.test_stencil_modes_bit_exact, (2, 15, 1), "... 2-D"),
    (K.test_sweep_with_input_residual_norm_bit_exact, (3, 31, 2), "mgk_jacobi_sumsq_f64"),
    (K.test_sweep_with_input_residual_norm_bit_exact, (2, 127, 0), "mgk_jacobi_sumsq_f64, 2-D"),
    (K.test_sweep_with_norm_over_plane_ranges, (31, 0), "mgk_jacobi_sumsq_range_f64 mgk_partials_finish"),
    (DK.test_sweep_over_plane_ranges, (3, 7), "mgk_jacobi_range_f64"),
    (DK.test_sweep_over_plane_ranges, (2, 255), "mgk_jacobi_range_f64, 2-D rows"),
    # B. 3-D fused, whole grid: generic forms on small cubes ...
    (K.test_two_sweeps_in_one_pass_bit_exact, (7,), "mgk_jacobi2_f64"),
    (K.test_two_sweeps_in_one_pass_bit_exact, (31,), "mgk_jacobi2_f64"),
    (K.test_fused_prolong_jacobi_bit_exact, (7, 0), "mgk_prolong_jacobi_f64"),
    (K.test_fused_prolong_jacobi_bit_exact, (31, 31), "mgk_prolong_jacobi_f64, the register form"),
    (K.test_fused_prolong_jacobi_2d_bit_exact, (7, 0), "mgk_prolong_jacobi_f64, 2-D"),
    (K.test_fused_prolong_jacobi_2d_bit_exact, (127, 38), "mgk_prolong_jacobi_f64, 2-D independent waves"),
    (K.test_fused_prolong_jacobi_plane_ranges, (31, 0, (2, 30)), "mgk_prolong_jacobi_range_f64"),
    (K.test_fused_prolong_jacobi_plane_ranges, (31, 31, (2, 30)), "mgk_prolong_jacobi_range_f64, the register form"),
    (K.test_fused_residual_restrict_bit_exact, (7,), "mgk_residual_restrict_f64 (variants 30, 31, 34 inside)"),
    (K.test_fused_residual_restrict_bit_exact, (15,), "mgk_residual_restrict_f64"),
    (K.test_fused_residual_restrict_coarse_plane_ranges, (15,), "mgk_residual_restrict_range_f64"),
    (K.test_fused_residual_restrict_with_coarse_first_sweep, (7,), "mgk_residual_restrict_jz_f64: uc0 follows the COARSE set"),
    # ... and the full-row forms (rows of 512 / 1024) on thin grids: every fine-level pass of the default cycle, scale 6/7
    (HW.test_sweeps_and_norms_against_the_oracle, (511, 5),
     "mgk_jacobi_f64 mgk_jacobi_sumsq_f64 mgk_residual_sumsq_f64 mgk_residual_f64 mgk_jacobi2_f64 mgk_jacobi2_sumsq_f64 mgk_jacobi2_sumsq_mid_f64 "
     "mgk_jacobi2_zero_f64"),
    (HW.test_sweeps_and_norms_against_the_oracle, (1023, 3), "... the 8-wave instances"),
    (HW.test_transfer_passes_against_the_oracle, (511, 5),
     "mgk_prolong_jacobi_f64 mgk_prolong_jacobi2_f64 mgk_residual_restrict_f64 mgk_residual_restrict_jz_f64 mgk_sweep_residual_restrict_f64"),
    (HW.test_transfer_passes_against_the_oracle, (1023, 3), "... the 8-wave instances"),
    (FM.test_interp_jacobi2_3d_equals_the_oracle, (511, 5), "mgk_interp_jacobi2_f64"),
    # C. slab forms that the other modules already compare with the oracle alone
    (DK.test_two_sweeps_on_z_slabs, (31, (0, 9, 31)), "mgk_jacobi2_slab_f64"),
    (K.test_fused_residual_restrict_on_slabs_single_exchange, (31, 7), "mgk_residual_restrict_slab_f64"),
    (K.test_fused_residual_restrict_on_slabs_single_exchange, (15, 2), "mgk_residual_restrict_slab_f64, one launch"),
    # D. 2-D
    (K.test_fused_residual_restrict_2d_bit_exact, (63,), "mgk_residual_restrict_2d_f64 (variants 55, 56 inside)"),
    (K.test_2d_forms_of_the_four_pass_kernels_bit_exact, (127,), "mgk_sweep_residual_restrict_2d_f64 mgk_jacobi2_2d_sumsq_f64"),
    (FM.test_interp_jacobi3_2d_equals_the_oracle, (127,), "mgk_interp_jacobi3_2d_f64"),
    # F. full multigrid in the LDS tail: tests/fmg_reference.py asks for one set per level
    (FM.test_tail_fmg_equals_the_restatement, (2, 31, 3, 1), "mgk_tail_fmg_f64"),
    (FM.test_tail_fmg_equals_the_restatement, (3, 15, 4, 2), "mgk_tail_fmg_f64, 3-D, nu = 2"),
    # G. fp32 and the bridges (scale 6/7; the oracle's *32 forms)
    (MX.test_fp32_kernels_bit_exact, (7,), "mgk_jacobi_f32 mgk_residual_f32"),
    (MX.test_fp32_kernels_bit_exact, (31,), "mgk_jacobi_f32 mgk_residual_f32"),
    (MX.test_two_fp32_sweeps_in_one_pass_bit_exact, (31,), "mgk_jacobi2_f32"),
    (MX.test_fused_residual_restrict_fp32_bit_exact, (31,), "mgk_residual_restrict_f32"),
    (MX.test_bridges_fp64_fp32, (7,), "mgk_residual_f64_to_f32"),
    (MX.test_fused_correction_and_residual_bit_exact, (31, 2), "mgk_correct_residual_f64_f32"),
    (MW.test_sweeps_at_width, (255, 255, 5), "mgk_jacobi_f32 mgk_residual_f32 mgk_jacobi2_f32 mgk_jacobi2_zero_f32, full rows"),
    (MW.test_transfers_at_width, (255, 255, 5), "mgk_prolong_jacobi_f32 mgk_residual_restrict_f32 mgk_residual_restrict_jz_f32"),
    (MW.test_bridges_at_width, (255, 5),
     "mgk_residual_f64_to_f32 mgk_residual_f64_to_f32_jz mgk_correct_residual_f64_f32 mgk_correct_residual_f64_f32_jz"),
    (MW.test_fp32_slab_forms, (255, 13, (0, 2, 6)),
     "mgk_jacobi_range_f32 mgk_residual_range_f32 mgk_jacobi2_slab_f32 mgk_prolong_jacobi_range_f32 mgk_residual_restrict_slab_f32 "
     "mgk_residual_restrict_range_f32"),
]


@pytest.mark.parametrize("body,args,covers", REUSED, ids=[f"{b.__module__[5:-4]}.{b.__name__[5:]}-{'-'.join(map(str, a))}".replace(" ", "") for b, a, _ in REUSED])
def test_oracle_pinned_body_on_distinct_coefficients(mgk, orc, body, args, covers):
    before = orc.served
    body(mgk, orc, *args)
    assert orc.served > before, "the body did not take its coefficients from the oracle object"


# ------------------------------------------------------------------------------------------------------------------------------
# A. single pass: what REUSED leaves (mgk_apply_f64, mgk_residual_range_f64), and every entry point again at scale 6/7
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n,variants", [(3, 7, ((-1, -1), (0, 5), (2, -1))), (3, 31, ((-1, -1), (2, 5))), (3, 63, ((1, -1), (6, 5))),
                                            (2, 15, ((-1, -1), (1, 5))), (2, 127, ((-1, -1), (0, 5), (1, -1))), (2, 255, ((2, -1),))])
def test_single_pass_kernels(mgk, orc, dim, n, variants):
    rng = np.random.default_rng(61000 + 10 * n + dim)
    As = distinct_coef(rng, dim)
    dinv = 1.0 / As[As.size // 2]
    sh = (n,) * dim
    u, b, pm = (dense_field(rng, *sh).ravel() for _ in range(3))
    j = orc.jacobi(dim, n, As, SC, b, u)
    r = orc.residual(dim, n, As, b, u)
    ch = orc.cheby_step(dim, n, As, b, u, pm, *CHEB)
    au = orc.apply(dim, n, As, u)
    L, g, d = mgk.L, mgk.geom(dim, n), Dev(mgk)
    gp, coef = C.byref(g), mgk.coef(As)
    du, db, dpm, o = d.field(g, u), d.field(g, b), d.field(g, pm), d.field(g)
    ss, npart = C.c_double(), C.c_int()
    ranges = ((1, n - 1), (0, 1), (n - 1, n))
    for var, zc in variants:
        L.mgk_set_tuning(var, zc)
        tag = f"variant={var} zc={zc}"
        d.zero(g, o)
        mgk._chk(L.mgk_jacobi_f64(mgk.ctx, gp, coef, dinv, SC, db, du, o, None))
        _same(mgk, g, o, j, f"mgk_jacobi_f64 {tag}")
        d.zero(g, o)
        mgk._chk(L.mgk_residual_f64(mgk.ctx, gp, coef, db, du, o, None))
        _same(mgk, g, o, r, f"mgk_residual_f64 {tag}")
        mgk._chk(L.mgk_residual_sumsq_f64(mgk.ctx, gp, coef, db, du, C.byref(ss), None))
        _red(orc, ss, r, f"mgk_residual_sumsq_f64 {tag}")
        d.zero(g, o)
        mgk._chk(L.mgk_cheby_f64(mgk.ctx, gp, coef, dinv, *CHEB, db, du, dpm, o, None))
        _same(mgk, g, o, ch, f"mgk_cheby_f64 {tag}")
        d.zero(g, o)
        mgk._chk(L.mgk_apply_f64(mgk.ctx, gp, coef, du, o, None))
        _same(mgk, g, o, au, f"mgk_apply_f64 {tag}")
        d.zero(g, o)
        mgk._chk(L.mgk_jacobi_sumsq_f64(mgk.ctx, gp, coef, dinv, SC, db, du, o, C.byref(ss), None))
        _same(mgk, g, o, j, f"mgk_jacobi_sumsq_f64 {tag}")
        _red(orc, ss, r, f"mgk_jacobi_sumsq_f64 {tag}")
        # the plane (2-D: row) ranges of a slab rank: interior first, then the two boundary ones
        d.zero(g, o)
        for z0, z1 in ranges:
            mgk._chk(L.mgk_jacobi_range_f64(mgk.ctx, gp, coef, dinv, SC, db, du, o, z0, z1, None))
        _same(mgk, g, o, j, f"mgk_jacobi_range_f64 {tag}")
        d.zero(g, o)
        for z0, z1 in ranges:
            mgk._chk(L.mgk_residual_range_f64(mgk.ctx, gp, coef, db, du, o, z0, z1, None))
        _same(mgk, g, o, r, f"mgk_residual_range_f64 {tag}")
        d.zero(g, o)
        off = 0
        for z0, z1 in ranges:
            mgk._chk(L.mgk_jacobi_sumsq_range_f64(mgk.ctx, gp, coef, dinv, SC, db, du, o, z0, z1, off, C.byref(npart), None))
            off += npart.value
        mgk._chk(L.mgk_partials_finish(mgk.ctx, off, C.byref(ss), None))
        _same(mgk, g, o, j, f"mgk_jacobi_sumsq_range_f64 {tag}")
        _red(orc, ss, r, f"mgk_jacobi_sumsq_range_f64 + mgk_partials_finish {tag}")
    L.mgk_set_tuning(-1, -1)
    for f, x in ((du, u), (db, b), (dpm, pm)):
        assert np.array_equal(mgk.from_field(g, f), x)
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------
# B. three sweeps per pass in 3-D (the module of these kernels builds its own uniform stencil)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nz", [(7, 7), (31, 31), (127, 5)])
def test_three_sweeps_3d(mgk, orc, n, nz):
    rng = np.random.default_rng(62000 + n)
    As = distinct_coef(rng, 3)
    dinv = 1.0 / As[3]
    u, b = dense_field(rng, nz * n * n), dense_field(rng, nz * n * n)
    J = lambda x: orc.jacobi(3, n, As, SC, b, x, nz=nz)
    want = J(J(J(u)))
    r0 = orc.residual(3, n, As, b, u, nz=nz)
    L, g, d = mgk.L, mgk.geom(3, n, n, nz), Dev(mgk)
    du, db, o = d.field(g, u), d.field(g, b), d.field(g)
    ss = C.c_double()
    for var, zc in ((-1, -1), (62, -1), (63, -1), (64, -1), (-1, 5), (63, 3)):          # tile heights 2 / 3 / 4, the row-by-row form, z chunks
        L.mgk_set_tuning(var, zc)
        d.zero(g, o)
        mgk._chk(L.mgk_jacobi3_f64(mgk.ctx, C.byref(g), mgk.coef(As), dinv, SC, db, du, o, None))
        _same(mgk, g, o, want, f"mgk_jacobi3_f64 variant={var} zc={zc}")
        d.zero(g, o)
        mgk._chk(L.mgk_jacobi3_sumsq_f64(mgk.ctx, C.byref(g), mgk.coef(As), dinv, SC, db, du, o, C.byref(ss), None))
        _same(mgk, g, o, want, f"mgk_jacobi3_sumsq_f64 variant={var} zc={zc}")
        _red(orc, ss, r0, f"mgk_jacobi3_sumsq_f64 variant={var} zc={zc}")
    L.mgk_set_tuning(-1, -1)
    assert np.array_equal(mgk.from_field(g, du), u) and np.array_equal(mgk.from_field(g, db), b)
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------
# C. slab forms whose own tests lean on the whole-grid kernels: here against the oracle's whole-grid result
# ------------------------------------------------------------------------------------------------------------------------------
def test_four_pass_kernels_on_slabs(mgk, orc):
    """mgk_sweep_residual_restrict_slab_f64 and mgk_jacobi2_sumsq_slab_f64 on three z-slabs of a 127^3 grid (ghost planes, far / far2 / bfar as
    the halo exchange delivers them; the plane ranges the solver launches): each slab's part of the oracle's swept field, coarse
    right-hand side and two-sweep field, and the norm partials summed over the slabs"""
    n, cuts = 127, (0, 20, 44, 63)
    rng = np.random.default_rng(63000)
    nc = (n - 1) // 2
    As = distinct_coef(rng, 3)
    dinv = 1.0 / As[3]
    u, b = dense_field(rng, n ** 3), dense_field(rng, n ** 3)
    w = orc.jacobi(3, n, As, SC, b, u)
    w_ref = w.reshape(n, n, n)
    bc_ref = orc.restrict(3, n, orc.residual(3, n, As, b, w)).reshape(nc, nc, nc)
    u2_ref = orc.jacobi(3, n, As, SC, b, w).reshape(n, n, n)
    r0 = orc.residual(3, n, As, b, u)
    L, coef = mgk.L, mgk.coef(As)
    U, B = u.reshape(n, n, n), b.reshape(n, n, n)
    total = 0.0
    for s in range(len(cuts) - 1):
        kc0, kc1 = cuts[s], cuts[s + 1]
        last = s == len(cuts) - 2
        z0, z1 = 2 * kc0, (n if last else 2 * kc1)
        nz, nzc = z1 - z0, kc1 - kc0
        has_lo, has_hi = int(s > 0), int(not last)
        gs, gcs, gfar = mgk.geom(3, n, n, nz), mgk.geom(3, nc, nc, nzc), mgk.geom(3, n, n, 2)
        assert L.mgk_sweep_residual_restrict_slab_ok_f64(C.byref(gs), C.byref(gcs)) == 1
        d = Dev(mgk)
        us, bs = d.keep(K._slab_field(mgk, gs, u, n, z0)), d.keep(K._slab_field(mgk, gs, b, n, z0))
        far = d.keep(K._far_field(mgk, gfar, n, U[z0 - 2] if has_lo else None, U[z1 + 1] if has_hi else None))
        far2 = d.keep(K._far_field(mgk, gfar, n, None, U[z1 + 2] if has_hi and z1 + 2 < n else None))
        bfar = d.keep(K._far_field(mgk, gfar, n, None, B[z1 + 1] if has_hi else None))
        out, bcs = d.field(gs), d.field(gcs)
        for k0, k1 in ((1, nzc - 2), (0, 1), (nzc - 2, nzc)):
            mgk._chk(L.mgk_sweep_residual_restrict_slab_f64(mgk.ctx, C.byref(gs), C.byref(gcs), C.byref(gfar), coef, dinv, SC, bs, us, out,
                                                            far, far2, bfar, has_lo, has_hi, bcs, k0, k1, None))
        _same(mgk, gs, out, w_ref[z0:z1], f"mgk_sweep_residual_restrict_slab_f64 slab {s}: swept field")
        _same(mgk, gcs, bcs, bc_ref[kc0:kc1], f"mgk_sweep_residual_restrict_slab_f64 slab {s}: coarse right-hand side")
        d.zero(gs, out)
        n1, off = C.c_int(0), 0
        for a0, a1 in ((2, nz - 2), (0, 2), (nz - 2, nz)):
            mgk._chk(L.mgk_jacobi2_sumsq_slab_f64(mgk.ctx, C.byref(gs), C.byref(gfar), coef, dinv, SC, bs, us, out, far, has_lo, has_hi,
                                                  a0, a1, off, C.byref(n1), None))
            off += n1.value
        ss = C.c_double(0.0)
        mgk._chk(L.mgk_partials_finish(mgk.ctx, off, C.byref(ss), None))
        total += ss.value
        _same(mgk, gs, out, u2_ref[z0:z1], f"mgk_jacobi2_sumsq_slab_f64 slab {s}")
        d.close()
    _red(orc, C.c_double(total), r0, "mgk_jacobi2_sumsq_slab_f64: norm over the slabs")


def test_ninety_one_byte_passes_on_slabs(mgk, orc):
    """mgk_prolong_jacobi2_slab_f64 and mgk_jacobi2_sumsq_mid_slab_f64 on three z-slabs of a thin 511 x 511 x 23 grid: each slab's part of
    the oracle's J(J(u + P uc)) and J(J(u)), and || b - A J(u) ||^2 summed over the slabs"""
    n, nzcw, cuts = 511, 11, (0, 3, 7, 11)
    rng = np.random.default_rng(64000)
    nc, nzw = (n - 1) // 2, 2 * nzcw + 1
    As = distinct_coef(rng, 3)
    dinv = 1.0 / As[3]
    L, coef = mgk.L, mgk.coef(As)
    U, B, UC = dense_field(rng, nzw, n, n), dense_field(rng, nzw, n, n), dense_field(rng, nzcw, nc, nc)
    J = lambda x: orc.jacobi(3, n, As, SC, B.ravel(), x, nz=nzw)
    pj_ref = J(J(orc.prolong_add(3, n, UC.ravel(), U.ravel(), nzf=nzw, nzc=nzcw))).reshape(nzw, n, n)
    j1 = J(U.ravel())
    j2_ref = J(j1).reshape(nzw, n, n)
    r1 = orc.residual(3, n, As, B.ravel(), j1, nz=nzw)
    total = 0.0
    for s in range(len(cuts) - 1):
        kc0, kc1 = cuts[s], cuts[s + 1]
        last = s == len(cuts) - 2
        z0, z1 = 2 * kc0, (nzw if last else 2 * kc1)
        nz, nzc = z1 - z0, kc1 - kc0
        has_lo, has_hi = int(s > 0), int(not last)
        gs, gcs, gfar, gcfar = mgk.geom(3, n, n, nz), mgk.geom(3, nc, nc, nzc), mgk.geom(3, n, n, 2), mgk.geom(3, nc, nc, 2)
        assert L.mgk_prolong_jacobi2_slab_ok_f64(C.byref(gs), C.byref(gcs), has_hi) == 1
        d = Dev(mgk)
        us, bs, ucs = (d.keep(K._thin_slab_field(mgk, gg, W, zz)) for gg, W, zz in ((gs, U, z0), (gs, B, z0), (gcs, UC, kc0)))
        far = d.keep(K._far_field(mgk, gfar, n, U[z0 - 2] if has_lo else None, U[z1 + 1] if has_hi else None))
        cfar = d.keep(K._far_field(mgk, gcfar, nc, UC[kc0 - 2] if has_lo and kc0 >= 2 else None, None))
        out = d.field(gs)
        zi0, zi1 = (4 if has_lo else 0), (nz - 2 if has_hi else nz)
        ranges = [(zi0, zi1)] + ([(0, 4)] if has_lo else []) + ([(nz - 2, nz)] if has_hi else [])
        for zc in (-1, 8):
            L.mgk_set_tuning(-1, zc)
            d.zero(gs, out)
            for a0, a1 in ranges:
                mgk._chk(L.mgk_prolong_jacobi2_slab_f64(mgk.ctx, C.byref(gs), C.byref(gcs), C.byref(gfar), C.byref(gcfar), coef, dinv, SC, bs, ucs, us,
                                                        out, far, cfar, has_lo, has_hi, a0, a1, None))
            _same(mgk, gs, out, pj_ref[z0:z1], f"mgk_prolong_jacobi2_slab_f64 slab {s} zc={zc}")
        L.mgk_set_tuning(-1, -1)
        d.zero(gs, out)
        n1, off = C.c_int(0), 0
        for a0, a1 in ((2, nz - 2), (0, 2), (nz - 2, nz)):
            mgk._chk(L.mgk_jacobi2_sumsq_mid_slab_f64(mgk.ctx, C.byref(gs), C.byref(gfar), coef, dinv, SC, bs, us, out, far, has_lo, has_hi,
                                                      a0, a1, off, C.byref(n1), None))
            off += n1.value
        sp = C.c_double(0.0)
        mgk._chk(L.mgk_partials_finish(mgk.ctx, off, C.byref(sp), None))
        total += sp.value
        _same(mgk, gs, out, j2_ref[z0:z1], f"mgk_jacobi2_sumsq_mid_slab_f64 slab {s}")
        d.close()
    _red(orc, C.c_double(total), r1, "mgk_jacobi2_sumsq_mid_slab_f64: norm over the slabs")


# ------------------------------------------------------------------------------------------------------------------------------
# D. 2-D fused passes on constant coefficients
# ------------------------------------------------------------------------------------------------------------------------------
# default; three-sweep forms forced (50 marching, 51 / 52 chunks of 4 / 8 rows); y chunks; residual + restriction forms (55, 56); waves (38)
VARIANTS_2D = ((-1, -1), (50, -1), (51, -1), (52, -1), (-1, 5), (55, -1), (56, -1), (38, 3), (58, 12))


@pytest.mark.parametrize("n", [15, 127, 255])
def test_2d_fused_passes_on_constant_coefficients(mgk, orc, n):
    rng = np.random.default_rng(65000 + n)
    nc = (n - 1) // 2
    As, Ac = distinct_coef(rng, 2, per_level=2)
    dinv, dinv_c = 1.0 / As[2], 1.0 / Ac[2]
    u, b, uc = dense_field(rng, n * n), dense_field(rng, n * n), dense_field(rng, nc * nc)
    J = lambda x, zg=False: orc.jacobi(2, n, As, SC, b, x, zero_guess=zg)
    Jc0 = lambda bc: orc.jacobi(2, nc, Ac, SC_C, bc, np.zeros_like(bc), zero_guess=True)      # the coarse level's first sweep: ITS constants
    j1 = J(u)
    j2 = J(j1)
    j3 = J(j2)
    z3 = J(J(J(np.zeros(n * n), True)))
    r0 = orc.residual(2, n, As, b, u)
    bc0 = orc.restrict(2, n, r0)
    bc1 = orc.restrict(2, n, orc.residual(2, n, As, b, j1))
    pu = orc.prolong_add(2, n, uc, u)
    pj3 = J(J(J(pu)))
    i3 = J(J(J(orc.prolong_add(2, n, uc, np.zeros(n * n)))))
    c7 = cheb7(*EIG)
    p3 = ksp_solve(orc, 2, n, As, b, u, 3, *EIG, zero=False)
    zc3 = ksp_solve(orc, 2, n, As, b, None, 3, *EIG, zero=True)
    pc3 = ksp_solve(orc, 2, n, As, b, pu, 3, *EIG, zero=False)
    L, d = mgk.L, Dev(mgk)
    gf, gc = mgk.geom(2, n), mgk.geom(2, nc)
    g, gcp, coef = C.byref(gf), C.byref(gc), mgk.coef(As)
    du, db, duc = d.field(gf, u), d.field(gf, b), d.field(gc, uc)
    o, rr, obc, ouc = d.field(gf), d.field(gf), d.field(gc), d.field(gc)
    ss = C.c_double()

    def fresh():
        d.zero(gf, o, rr)
        d.zero(gc, obc, ouc)
    for var, zc in VARIANTS_2D:
        L.mgk_set_tuning(var, zc)
        t = f"variant={var} zc={zc}"
        fresh()
        mgk._chk(L.mgk_jacobi2_2d_f64(mgk.ctx, g, coef, dinv, SC, db, du, o, None))
        _same(mgk, gf, o, j2, f"mgk_jacobi2_2d_f64 {t}")
        fresh()
        mgk._chk(L.mgk_jacobi2_2d_sumsq_f64(mgk.ctx, g, coef, dinv, SC, db, du, o, C.byref(ss), None))
        _same(mgk, gf, o, j2, f"mgk_jacobi2_2d_sumsq_f64 {t}")
        _red(orc, ss, r0, f"mgk_jacobi2_2d_sumsq_f64 {t}")
        fresh()
        mgk._chk(L.mgk_residual_restrict_2d_f64(mgk.ctx, g, gcp, coef, db, du, obc, ouc, dinv_c, SC_C, None))
        _same(mgk, gc, obc, bc0, f"mgk_residual_restrict_2d_f64 {t}: coarse right-hand side")
        _same(mgk, gc, ouc, Jc0(bc0), f"mgk_residual_restrict_2d_f64 {t}: coarse first sweep")
        fresh()
        mgk._chk(L.mgk_sweep_residual_restrict_2d_f64(mgk.ctx, g, gcp, coef, dinv, SC, db, du, o, obc, ouc, dinv_c, SC_C, None))
        _same(mgk, gf, o, j1, f"mgk_sweep_residual_restrict_2d_f64 {t}: swept field")
        _same(mgk, gc, obc, bc1, f"mgk_sweep_residual_restrict_2d_f64 {t}: coarse right-hand side")
        _same(mgk, gc, ouc, Jc0(bc1), f"mgk_sweep_residual_restrict_2d_f64 {t}: coarse first sweep")
        fresh()
        mgk._chk(L.mgk_jacobi_sumsq_store_f64(mgk.ctx, g, coef, dinv, SC, None, None, db, du, o, rr, C.byref(ss), None))
        _same(mgk, gf, o, j1, f"mgk_jacobi_sumsq_store_f64 {t}: sweep")
        _same(mgk, gf, rr, r0, f"mgk_jacobi_sumsq_store_f64 {t}: stored residual")
        _red(orc, ss, r0, f"mgk_jacobi_sumsq_store_f64 {t}")
        fresh()
        mgk._chk(L.mgk_jacobi3_2d_f64(mgk.ctx, g, coef, dinv, SC, None, None, db, du, o, None))
        _same(mgk, gf, o, j3, f"mgk_jacobi3_2d_f64 {t}")
        fresh()
        mgk._chk(L.mgk_jacobi3_2d_sumsq_f64(mgk.ctx, g, coef, dinv, SC, None, None, db, du, o, C.byref(ss), None))
        _same(mgk, gf, o, j3, f"mgk_jacobi3_2d_sumsq_f64 {t}")
        _red(orc, ss, r0, f"mgk_jacobi3_2d_sumsq_f64 {t}")
        fresh()
        mgk._chk(L.mgk_jacobi3_2d_sumsq_store_f64(mgk.ctx, g, coef, dinv, SC, None, None, db, du, o, rr, C.byref(ss), None))
        _same(mgk, gf, o, j3, f"mgk_jacobi3_2d_sumsq_store_f64 {t}: three sweeps")
        _same(mgk, gf, rr, r0, f"mgk_jacobi3_2d_sumsq_store_f64 {t}: stored residual")
        _red(orc, ss, r0, f"mgk_jacobi3_2d_sumsq_store_f64 {t}")
        fresh()
        mgk._chk(L.mgk_jacobi3_2d_zero_f64(mgk.ctx, g, coef, dinv, SC, None, None, db, o, None))
        _same(mgk, gf, o, z3, f"mgk_jacobi3_2d_zero_f64 {t}")
        fresh()
        mgk._chk(L.mgk_prolong_jacobi3_2d_f64(mgk.ctx, g, gcp, coef, dinv, SC, None, None, db, duc, du, o, None))
        _same(mgk, gf, o, pj3, f"mgk_prolong_jacobi3_2d_f64 {t}")
        fresh()
        mgk._chk(L.mgk_interp_jacobi3_2d_f64(mgk.ctx, g, gcp, coef, dinv, SC, db, duc, o, None))
        _same(mgk, gf, o, i3, f"mgk_interp_jacobi3_2d_f64 {t}")
        fresh()
        mgk._chk(L.mgk_cheby3_2d_f64(mgk.ctx, g, coef, dinv, _dp(c7), None, None, db, du, o, None))
        _same(mgk, gf, o, p3, f"mgk_cheby3_2d_f64 {t}")
        fresh()
        mgk._chk(L.mgk_cheby3_2d_sumsq_f64(mgk.ctx, g, coef, dinv, _dp(c7), None, None, db, du, o, C.byref(ss), None))
        _same(mgk, gf, o, p3, f"mgk_cheby3_2d_sumsq_f64 {t}")
        _red(orc, ss, r0, f"mgk_cheby3_2d_sumsq_f64 {t}")
        fresh()
        mgk._chk(L.mgk_cheby3_2d_zero_f64(mgk.ctx, g, coef, dinv, _dp(c7), None, None, db, o, None))
        _same(mgk, gf, o, zc3, f"mgk_cheby3_2d_zero_f64 {t}")
        fresh()
        mgk._chk(L.mgk_prolong_cheby3_2d_f64(mgk.ctx, g, gcp, coef, dinv, _dp(c7), None, None, db, duc, du, o, None))
        _same(mgk, gf, o, pc3, f"mgk_prolong_cheby3_2d_f64 {t}")
    L.mgk_set_tuning(-1, -1)
    assert np.array_equal(mgk.from_field(gf, du), u) and np.array_equal(mgk.from_field(gf, db), b) and np.array_equal(mgk.from_field(gc, duc), uc)
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------
# E. row tables with W != E: against tests/row_tables.py (numpy, canonical order)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 127])
def test_row_table_kernels_with_west_unlike_east(mgk, orc, n):
    rng = np.random.default_rng(66000 + n)
    nc = (n - 1) // 2
    ct, dt = distinct_row_tables(rng, n)
    ctc, dtc = distinct_row_tables(rng, nc)
    U, B, PM, UC = dense_field(rng, n, n), dense_field(rng, n, n), dense_field(rng, n, n), dense_field(rng, nc, nc)
    A = lambda x: _rt_apply(ct, x)
    J = lambda x: _rt_jacobi(ct, B, x, SC)
    R = lambda r: orc.restrict(2, n, np.ascontiguousarray(r).ravel()).reshape(nc, nc)
    Jc0 = lambda bc: SC_C * (bc * dtc[:, None])
    j1 = J(U)
    j2 = J(j1)
    j3 = J(j2)
    r0 = B - A(U)
    z1 = SC * (B * dt[:, None])
    z3 = J(J(z1))
    bc0, bc1 = R(r0), R(B - A(j1))
    pu = orc.prolong_add(2, n, UC.ravel(), U.ravel()).reshape(n, n)
    ch = (CHEB[0] * PM + CHEB[1] * U) + CHEB[2] * (r0 * dt[:, None])
    c7 = cheb7(*EIG)
    p3 = ksp_solve_rt(ct, dt, B, U, 3, *EIG, zero=False)
    zc3 = ksp_solve_rt(ct, dt, B, None, 3, *EIG, zero=True)
    pc3 = ksp_solve_rt(ct, dt, B, pu, 3, *EIG, zero=False)
    L, d = mgk.L, Dev(mgk)
    gf, gc = mgk.geom(2, n), mgk.geom(2, nc)
    g, gcp = C.byref(gf), C.byref(gc)
    du, db, dpm, duc = d.field(gf, U), d.field(gf, B), d.field(gf, PM), d.field(gc, UC)
    dct, ddt, ddtc = d.up(ct), d.up(dt), d.up(dtc)
    o, rr, obc, ouc = d.field(gf), d.field(gf), d.field(gc), d.field(gc)
    ss = C.c_double()

    def fresh():
        d.zero(gf, o, rr)
        d.zero(gc, obc, ouc)
    for var, zc in ((-1, -1), (50, -1), (51, -1), (52, -1), (-1, 5), (38, 5), (58, 16)):
        L.mgk_set_tuning(var, zc)
        t = f"variant={var} zc={zc}"
        for mode, want in ((0, j1), (1, r0), (4, A(U))):
            fresh()
            mgk._chk(L.mgk_rowcoef_f64(mgk.ctx, g, mode, dct, ddt if mode == 0 else None, SC, None if mode == 4 else db, du, o, None))
            _same(mgk, gf, o, want, f"mgk_rowcoef_f64 mode {mode} {t}")
        fresh()
        mgk._chk(L.mgk_cheby_rowcoef_f64(mgk.ctx, g, dct, ddt, *CHEB, db, du, dpm, o, None))
        _same(mgk, gf, o, ch, f"mgk_cheby_rowcoef_f64 {t}")
        fresh()
        mgk._chk(L.mgk_jacobi_zero_rowcoef_f64(mgk.ctx, g, ddt, SC, db, o, None))
        _same(mgk, gf, o, z1, f"mgk_jacobi_zero_rowcoef_f64 {t}")
        fresh()
        mgk._chk(L.mgk_jacobi2_2d_rowcoef_f64(mgk.ctx, g, dct, ddt, SC, db, du, o, None))
        _same(mgk, gf, o, j2, f"mgk_jacobi2_2d_rowcoef_f64 {t}")
        fresh()
        mgk._chk(L.mgk_jacobi_sumsq_rowcoef_f64(mgk.ctx, g, dct, ddt, SC, db, du, o, C.byref(ss), None))
        _same(mgk, gf, o, j1, f"mgk_jacobi_sumsq_rowcoef_f64 {t}")
        _red(orc, ss, r0, f"mgk_jacobi_sumsq_rowcoef_f64 {t}")
        mgk._chk(L.mgk_residual_sumsq_rowcoef_f64(mgk.ctx, g, dct, db, du, C.byref(ss), None))
        _red(orc, ss, r0, f"mgk_residual_sumsq_rowcoef_f64 {t}")
        fresh()
        mgk._chk(L.mgk_prolong_jacobi_rowcoef_f64(mgk.ctx, g, gcp, dct, ddt, SC, db, duc, du, o, None))
        _same(mgk, gf, o, J(pu), f"mgk_prolong_jacobi_rowcoef_f64 {t}")
        fresh()
        mgk._chk(L.mgk_residual_restrict_2d_rowcoef_f64(mgk.ctx, g, gcp, dct, db, du, obc, ouc, ddtc, SC_C, None))
        _same(mgk, gc, obc, bc0, f"mgk_residual_restrict_2d_rowcoef_f64 {t}: coarse right-hand side")
        _same(mgk, gc, ouc, Jc0(bc0), f"mgk_residual_restrict_2d_rowcoef_f64 {t}: coarse first sweep (the coarse level's 1/diag table)")
        fresh()
        mgk._chk(L.mgk_jacobi2_2d_sumsq_rowcoef_f64(mgk.ctx, g, dct, ddt, SC, db, du, o, C.byref(ss), None))
        _same(mgk, gf, o, j2, f"mgk_jacobi2_2d_sumsq_rowcoef_f64 {t}")
        _red(orc, ss, r0, f"mgk_jacobi2_2d_sumsq_rowcoef_f64 {t}")
        fresh()
        mgk._chk(L.mgk_sweep_residual_restrict_2d_rowcoef_f64(mgk.ctx, g, gcp, dct, ddt, SC, db, du, o, obc, ouc, ddtc, SC_C, None))
        _same(mgk, gf, o, j1, f"mgk_sweep_residual_restrict_2d_rowcoef_f64 {t}: swept field")
        _same(mgk, gc, obc, bc1, f"mgk_sweep_residual_restrict_2d_rowcoef_f64 {t}: coarse right-hand side")
        _same(mgk, gc, ouc, Jc0(bc1), f"mgk_sweep_residual_restrict_2d_rowcoef_f64 {t}: coarse first sweep")
        # the ctab / dtab arm of the entry points that take either form (coef = NULL, dinv ignored)
        fresh()
        mgk._chk(L.mgk_jacobi_sumsq_store_f64(mgk.ctx, g, None, 1.0, SC, dct, ddt, db, du, o, rr, C.byref(ss), None))
        _same(mgk, gf, o, j1, f"mgk_jacobi_sumsq_store_f64 tables {t}: sweep")
        _same(mgk, gf, rr, r0, f"mgk_jacobi_sumsq_store_f64 tables {t}: stored residual")
        _red(orc, ss, r0, f"mgk_jacobi_sumsq_store_f64 tables {t}")
        fresh()
        mgk._chk(L.mgk_jacobi3_2d_f64(mgk.ctx, g, None, 1.0, SC, dct, ddt, db, du, o, None))
        _same(mgk, gf, o, j3, f"mgk_jacobi3_2d_f64 tables {t}")
        fresh()
        mgk._chk(L.mgk_jacobi3_2d_sumsq_f64(mgk.ctx, g, None, 1.0, SC, dct, ddt, db, du, o, C.byref(ss), None))
        _same(mgk, gf, o, j3, f"mgk_jacobi3_2d_sumsq_f64 tables {t}")
        _red(orc, ss, r0, f"mgk_jacobi3_2d_sumsq_f64 tables {t}")
        fresh()
        mgk._chk(L.mgk_jacobi3_2d_sumsq_store_f64(mgk.ctx, g, None, 1.0, SC, dct, ddt, db, du, o, rr, C.byref(ss), None))
        _same(mgk, gf, o, j3, f"mgk_jacobi3_2d_sumsq_store_f64 tables {t}: three sweeps")
        _same(mgk, gf, rr, r0, f"mgk_jacobi3_2d_sumsq_store_f64 tables {t}: stored residual")
        _red(orc, ss, r0, f"mgk_jacobi3_2d_sumsq_store_f64 tables {t}")
        fresh()
        mgk._chk(L.mgk_jacobi3_2d_zero_f64(mgk.ctx, g, None, 1.0, SC, dct, ddt, db, o, None))
        _same(mgk, gf, o, z3, f"mgk_jacobi3_2d_zero_f64 tables {t}")
        fresh()
        mgk._chk(L.mgk_prolong_jacobi3_2d_f64(mgk.ctx, g, gcp, None, 1.0, SC, dct, ddt, db, duc, du, o, None))
        _same(mgk, gf, o, J(J(J(pu))), f"mgk_prolong_jacobi3_2d_f64 tables {t}")
        fresh()
        mgk._chk(L.mgk_cheby3_2d_f64(mgk.ctx, g, None, 1.0, _dp(c7), dct, ddt, db, du, o, None))
        _same(mgk, gf, o, p3, f"mgk_cheby3_2d_f64 tables {t}")
        fresh()
        mgk._chk(L.mgk_cheby3_2d_sumsq_f64(mgk.ctx, g, None, 1.0, _dp(c7), dct, ddt, db, du, o, C.byref(ss), None))
        _same(mgk, gf, o, p3, f"mgk_cheby3_2d_sumsq_f64 tables {t}")
        _red(orc, ss, r0, f"mgk_cheby3_2d_sumsq_f64 tables {t}")
        fresh()
        mgk._chk(L.mgk_cheby3_2d_zero_f64(mgk.ctx, g, None, 1.0, _dp(c7), dct, ddt, db, o, None))
        _same(mgk, gf, o, zc3, f"mgk_cheby3_2d_zero_f64 tables {t}")
        fresh()
        mgk._chk(L.mgk_prolong_cheby3_2d_f64(mgk.ctx, g, gcp, None, 1.0, _dp(c7), dct, ddt, db, duc, du, o, None))
        _same(mgk, gf, o, pc3, f"mgk_prolong_cheby3_2d_f64 tables {t}")
    L.mgk_set_tuning(-1, -1)
    for f, gg, x in ((du, gf, U), (db, gf, B), (dpm, gf, PM), (duc, gc, UC)):
        assert np.array_equal(mgk.from_field(gg, f), x.ravel())
    d.close()


# ------------------------------------------------------------------------------------------------------------------------------
# F. the LDS tails: another set (another pair of tables) on every level
# ------------------------------------------------------------------------------------------------------------------------------
def _levels(n0, nlev):
    ns = [n0]
    for _ in range(nlev - 1):
        ns.append((ns[-1] - 1) // 2)
    assert ns[-1] >= 1
    return ns


def _coef7(Ass, dim):
    k7 = np.zeros(7 * len(Ass))
    for l, As in enumerate(Ass):
        k7[7 * l:7 * l + As.size] = As
    return k7, np.array([1.0 / As[As.size // 2] for As in Ass])


def _tables_on_device(d, tabs):
    bufs = [(d.up(ct), d.up(dt)) for ct, dt in tabs]
    cta = (C.c_void_p * len(tabs))(*[C.cast(a, C.c_void_p).value for a, _ in bufs])
    dta = (C.c_void_p * len(tabs))(*[C.cast(x, C.c_void_p).value for _, x in bufs])
    return cta, dta


@pytest.mark.parametrize("dim,n0,nlev,v0,v1", [(2, 63, 6, 3, 3), (2, 15, 3, 2, 1), (3, 15, 4, 3, 3), (3, 7, 2, 1, 4)])
def test_tail_cycle_with_a_set_per_level(mgk, orc, dim, n0, nlev, v0, v1):
    """mgk_tail_cycle_f64 against the oracle's operators walked over the tail levels (tests/test_dropin_kernels_gpu.py::_tail_ref)"""
    rng = np.random.default_rng(67000 + 100 * dim + n0 + v1)
    ns = _levels(n0, nlev)
    Ass = distinct_coef(rng, dim, per_level=nlev)
    b0 = dense_field(rng, n0 ** dim)
    want = DK._tail_ref(ns, b0,
                        lambda l, b, u: orc.jacobi(dim, ns[l], Ass[l], SC, b, u),
                        lambda l, b: orc.jacobi(dim, ns[l], Ass[l], SC, b, np.zeros_like(b), zero_guess=True),
                        lambda l, b, u: orc.residual(dim, ns[l], Ass[l], b, u),
                        lambda l, r: orc.restrict(dim, ns[l], r),
                        lambda l, uc, uf: orc.prolong_add(dim, ns[l], uc, uf), v0, v1)
    g, d = mgk.geom(dim, n0), Dev(mgk)
    db, du = d.field(g, b0), d.field(g)
    k7, di = _coef7(Ass, dim)
    mgk._chk(mgk.L.mgk_tail_cycle_f64(mgk.ctx, C.byref(g), nlev, (C.c_int * nlev)(*ns), _dp(k7), _dp(di), SC, v0, v1, db, du, None))
    _same(mgk, g, du, want, "mgk_tail_cycle_f64")
    assert np.array_equal(mgk.from_field(g, db), b0)
    d.close()


@pytest.mark.parametrize("dim,n0,nlev,v0,v1", [(2, 31, 5, 3, 3), (2, 7, 2, 2, 1), (3, 15, 4, 3, 3), (3, 7, 3, 1, 4)])
def test_cheby_tail_with_a_set_per_level(mgk, orc, dim, n0, nlev, v0, v1):
    """mgk_tail_cycle_cheby_f64, the coef7 arm: every KSPSolve the restarted recurrence (tests/cheby_reference.py)"""
    rng = np.random.default_rng(68000 + 100 * dim + n0)
    ns = _levels(n0, nlev)
    Ass = distinct_coef(rng, dim, per_level=nlev)
    b0 = dense_field(rng, n0 ** dim)
    B, U = [b0], []
    for l in range(nlev):
        U.append(ksp_solve(orc, dim, ns[l], Ass[l], B[l], None, v1 if l == nlev - 1 else v0, *EIG, zero=True))
        if l < nlev - 1:
            B.append(orc.restrict(dim, ns[l], orc.residual(dim, ns[l], Ass[l], B[l], U[l])))
    for l in range(nlev - 2, -1, -1):
        U[l] = ksp_solve(orc, dim, ns[l], Ass[l], B[l], orc.prolong_add(dim, ns[l], U[l + 1], U[l]), v0, *EIG, zero=False)
    g, d = mgk.geom(dim, n0), Dev(mgk)
    db, du = d.field(g, b0), d.field(g)
    k7, di = _coef7(Ass, dim)
    mgk._chk(mgk.L.mgk_tail_cycle_cheby_f64(mgk.ctx, C.byref(g), nlev, (C.c_int * nlev)(*ns), _dp(k7), _dp(di), None, None, *EIG, v0, v1, db, du, None))
    _same(mgk, g, du, U[0], "mgk_tail_cycle_cheby_f64 (coef7)")
    d.close()


@pytest.mark.parametrize("n0,nlev,v0,v1,scale,cscale", [(63, 5, 3, 3, SC, SC), (15, 3, 2, 2, 0.7, 0.6), (31, 5, 3, 1, SC, 1.0)])
def test_row_table_tails_with_west_unlike_east(mgk, orc, n0, nlev, v0, v1, scale, cscale):
    """mgk_tail_cycle_rowcoef_f64 (cscale == scale), the row-table arm of mgk_tail_cycle_cs_f64, and the row-table arm of
    mgk_tail_cycle_cheby_f64, each level with its own tables: 1 / diag differs from row to row and from level to level"""
    rng = np.random.default_rng(69000 + n0)
    ns = _levels(n0, nlev)
    tabs = [distinct_row_tables(rng, n) for n in ns]
    b0 = dense_field(rng, n0, n0)
    sc = lambda l: cscale if l == nlev - 1 else scale
    restrict = lambda l, r: orc.restrict(2, ns[l], np.ascontiguousarray(r).ravel()).reshape(ns[l + 1], ns[l + 1])
    prolong = lambda l, uc, uf: orc.prolong_add(2, ns[l], uc.ravel(), uf.ravel()).reshape(ns[l], ns[l])
    want = DK._tail_ref(ns, b0,
                        lambda l, b, u: u + sc(l) * ((b - _rt_apply(tabs[l][0], u)) * tabs[l][1][:, None]),
                        lambda l, b: sc(l) * (b * tabs[l][1][:, None]),
                        lambda l, b, u: b - _rt_apply(tabs[l][0], u), restrict, prolong, v0, v1)
    g, d = mgk.geom(2, n0), Dev(mgk)
    db, du = d.field(g, b0), d.field(g)
    cta, dta = _tables_on_device(d, tabs)
    nn = (C.c_int * nlev)(*ns)
    mgk._chk(mgk.L.mgk_tail_cycle_cs_f64(mgk.ctx, C.byref(g), nlev, nn, None, None, cta, dta, scale, cscale, v0, v1, db, du, None))
    _same(mgk, g, du, want, "mgk_tail_cycle_cs_f64 (row tables)")
    if cscale == scale:
        d.zero(g, du)
        mgk._chk(mgk.L.mgk_tail_cycle_rowcoef_f64(mgk.ctx, C.byref(g), nlev, nn, cta, dta, scale, v0, v1, db, du, None))
        _same(mgk, g, du, want, "mgk_tail_cycle_rowcoef_f64")
    # Chebyshev on the same tables
    B, U = [b0], []
    for l in range(nlev):
        U.append(ksp_solve_rt(*tabs[l], B[l], None, v1 if l == nlev - 1 else v0, *EIG, zero=True))
        if l < nlev - 1:
            B.append(restrict(l, B[l] - _rt_apply(tabs[l][0], U[l])))
    for l in range(nlev - 2, -1, -1):
        U[l] = ksp_solve_rt(*tabs[l], B[l], prolong(l, U[l + 1], U[l]), v0, *EIG, zero=False)
    d.zero(g, du)
    mgk._chk(mgk.L.mgk_tail_cycle_cheby_f64(mgk.ctx, C.byref(g), nlev, nn, None, None, cta, dta, *EIG, v0, v1, db, du, None))
    _same(mgk, g, du, U[0], "mgk_tail_cycle_cheby_f64 (row tables)")
    assert np.array_equal(mgk.from_field(g, db), b0.ravel())
    d.close()
