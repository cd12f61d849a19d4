"""The bodies of the kernel-level GPU modules once more, on guarded and poisoned buffers (tests/guarded.py).

Those modules pin the INTERIOR of every kernel's output to the CPU oracle bit for bit.  Where a kernel's stores land they see only through
mgk_unpack_f64, and their outputs start zero-filled and are reused over the tuning variants.  Here the same bodies -- same calls, variants and
assertions -- run as body(Guarded(mgk), orc, *args): every allocation between two guard zones, the layout done on the host without
mgk_pack_* / mgk_unpack_*, every field(g) / field32(g) output poisoned with NaN, and every from_field* asserting that the ghost ring and the row
padding of the allocation are zero.  The contract this pins is the one of include/mgk.h, Conventions (quoted in tests/guarded.py).

CASES: (body, args, covers) -- covers: the entry points the case is there for; each must appear in the proxy's call log and, at least once, be
handed an output that still holds the poison (many bodies clear their outputs with mgk_memset0 and reuse them: the proxy poisons them again).
Before every call of a reducing entry point (guarded.REDUCERS) the proxy fills the context's whole reduction scratch with the poison too: a partial
slot that the finishing kernel adds up and the launch did not write turns the sum the body compares into NaN (tests/test_reduction_scratch_gpu.py).
The exceptions are tables with reasons: UNPOISONED (cases that run with the poison off: a body that asserts the zeros of its own memset), IN_PLACE
(entry points whose field is input and output at once, or whose output is no field), OWN_FRAMES and OWN_FILL (bodies that lay their own sentinels
instead).  Shapes: per
body the smallest parametrisations that reach each dispatch form (thin 511 x 511 x 5 and 1023 x 1023 x 3 grids for the full-row 3-D forms,
255 x 255 x 5 for fp32, 119 / 121 / 239 / 241 for the 2-D waves of 60 column pairs, 255 / 511 for the 2-D tiles of k_stencil, tails up to
mgk_tail_max_n); never a size of the benchmark's workload.  tests/test_guarded_cpu.py runs the same list over the host stand-ins and holds the
completeness gate: every entry point of include/mgk.h with a writable device-field parameter is in some case's covers, or in EXEMPT.

Written here: one body for the range forms (a finite sentinel outside the range must survive bitwise) and one for the layout
(mgk_pack_* / mgk_unpack_* against offset = org + k*plane + i*pitch + j written out in numpy)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import test_cheby3_kernels_gpu as CH
import test_distinct_coef_gpu as DC
import test_dropin_kernels_gpu as DK
import test_fmg_gpu as FM
import test_gmres_kernels_gpu as GM
import test_headline_width_gpu as HW
import test_kernels_gpu as K
import test_mixed_gpu as MX
import test_mixed_width_gpu as MW
import test_three_sweeps_gpu as T3
from guarded import EXEMPT, REDUCERS, Guarded, layout          # EXEMPT: the field writers no case here is there for, with the reasons
from multigrid_petsc_amd.mgk import Geom
from oracle import Oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RED_RTOL = 1e-13          # the project's figure for sums of squares (tests/test_kernels_gpu.py)
FILL = 12345.6789         # what the range body puts into the output before a call


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _w(s):
    return frozenset(s.split())


# ------------------------------------------------------------------------------------------------------------------------------
# the range forms: one call on a range that is not the whole grid, into an output whose interior holds FILL
# ------------------------------------------------------------------------------------------------------------------------------
def _ranges(n):
    """an inner range and one that touches each end"""
    return ((n // 4, n // 4 + max(1, n // 3)), (0, max(1, n // 10)), (n - max(1, n // 10), n))


def body_range_forms(mgk, orc, dim, nx, nz):
    """mgk_jacobi_range_*, mgk_residual_range_*, mgk_jacobi_sumsq_range_f64, mgk_prolong_jacobi_range_*, mgk_residual_restrict_range_* on the grid
    nx x nx (x nz): the planes / rows inside the range equal the oracle, every one outside is bitwise FILL, the frame is zero"""
    rng = np.random.default_rng(71000 + 10 * nx + nz)
    L, scale = mgk.L, 0.8
    ny = nx
    nm = nz if dim == 3 else ny                                   # length of the marching axis
    As = orc.level_stencil(dim, nx + 2, 0)[0]
    dinv = 1.0 / As[As.size // 2]
    N = nx * ny * (nz if dim == 3 else 1)
    kw = {"nz": nz} if dim == 3 else {}
    u, b = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    g = mgk.geom(dim, nx, ny, nz if dim == 3 else 1)
    gp, coef = C.byref(g), mgk.coef(As)
    du, db = mgk.to_field(g, u), mgk.to_field(g, b)
    own = [du, db]
    j, r = orc.jacobi(dim, nx, As, scale, b, u, **kw), orc.residual(dim, nx, As, b, u, **kw)

    def planes(x, m):
        return np.asarray(x).reshape(m, -1)

    def check(got, want, m, z0, z1, what):
        got, want = planes(got, m), planes(want, m)
        assert np.array_equal(got[z0:z1], want[z0:z1]), f"{what} [{z0}, {z1}): {np.count_nonzero(got[z0:z1] != want[z0:z1])} cells inside the range differ"
        bits = lambda a: np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)
        touched = np.flatnonzero(np.any(bits(got) != bits(np.full(1, FILL, dtype=got.dtype))[0], axis=1))
        outside = [int(q) for q in touched if not z0 <= q < z1]
        assert not outside, f"{what} [{z0}, {z1}): planes / rows outside the range were written: {outside[:8]}"

    ss, npart = C.c_double(), C.c_int()
    for z0, z1 in _ranges(nm):
        o = mgk.to_field(g, np.full(N, FILL))
        mgk._chk(L.mgk_jacobi_range_f64(mgk.ctx, gp, coef, dinv, scale, db, du, o, z0, z1, None))
        check(mgk.from_field(g, o), j, nm, z0, z1, "mgk_jacobi_range_f64")
        mgk.free(o)
        o = mgk.to_field(g, np.full(N, FILL))
        mgk._chk(L.mgk_residual_range_f64(mgk.ctx, gp, coef, db, du, o, z0, z1, None))
        check(mgk.from_field(g, o), r, nm, z0, z1, "mgk_residual_range_f64")
        mgk.free(o)
        o = mgk.to_field(g, np.full(N, FILL))
        ss.value = np.nan
        mgk._chk(L.mgk_jacobi_sumsq_range_f64(mgk.ctx, gp, coef, dinv, scale, db, du, o, z0, z1, 0, C.byref(npart), None))
        mgk._chk(L.mgk_partials_finish(mgk.ctx, npart.value, C.byref(ss), None))
        check(mgk.from_field(g, o), j, nm, z0, z1, "mgk_jacobi_sumsq_range_f64")
        ref = orc.sumsq(np.ascontiguousarray(planes(r, nm)[z0:z1]).ravel())
        assert abs(ss.value - ref) <= RED_RTOL * ref, f"mgk_jacobi_sumsq_range_f64 [{z0}, {z1}): {ss.value} vs {ref}"
        mgk.free(o)
    if dim == 3:
        nxc, nzc = (nx - 1) // 2, (nz - 1) // 2
        Nc = nxc * nxc * nzc
        uc = rng.uniform(-1, 1, Nc)
        gc = mgk.geom(3, nxc, nxc, nzc)
        gcp = C.byref(gc)
        duc = mgk.to_field(gc, uc)
        own.append(duc)
        pj = orc.jacobi(3, nx, As, scale, b, orc.prolong_add(3, nx, uc, u, nzf=nz, nzc=nzc), nz=nz)
        rr = orc.restrict(3, nx, r, nzf=nz, nzc=nzc)
        for z0, z1 in _ranges(nz):
            o = mgk.to_field(g, np.full(N, FILL))
            mgk._chk(L.mgk_prolong_jacobi_range_f64(mgk.ctx, gp, gcp, coef, dinv, scale, db, duc, du, o, z0, z1, None))
            check(mgk.from_field(g, o), pj, nz, z0, z1, "mgk_prolong_jacobi_range_f64")
            mgk.free(o)
        for k0, k1 in _ranges(nzc):
            o = mgk.to_field(gc, np.full(Nc, FILL))
            mgk._chk(L.mgk_residual_restrict_range_f64(mgk.ctx, gp, gcp, coef, db, du, o, k0, k1, None))
            check(mgk.from_field(gc, o), rr, nzc, k0, k1, "mgk_residual_restrict_range_f64")
            mgk.free(o)
        # fp32: the same fields rounded once, the oracle's fp32 leg on the thin grid
        u32, b32, uc32 = u.astype(np.float32), b.astype(np.float32), uc.astype(np.float32)
        g32, gc32 = Geom(), Geom()
        mgk._chk(L.mgk_geom_init_f32(C.byref(g32), 3, nx, ny, nz))
        mgk._chk(L.mgk_geom_init_f32(C.byref(gc32), 3, nxc, nxc, nzc))
        g32p, gc32p = C.byref(g32), C.byref(gc32)
        du32, db32, duc32 = mgk.to_field32(g32, u32), mgk.to_field32(g32, b32), mgk.to_field32(gc32, uc32)
        own += [du32, db32, duc32]
        j32 = orc.jacobi32(nx, As, scale, b32, u32, nz=nz, ny=ny)
        r32 = orc.residual32(nx, As, b32, u32, nz=nz, ny=ny)
        pj32 = orc.jacobi32(nx, As, scale, b32, orc.prolong_add32(nx, uc32, u32, nzf=nz, nzc=nzc, nyf=ny), nz=nz, ny=ny)
        rr32 = orc.restrict32(nx, r32, nzf=nz, nzc=nzc, nyf=ny)
        fill32, fillc32 = np.full(N, FILL, dtype=np.float32), np.full(Nc, FILL, dtype=np.float32)
        for z0, z1 in _ranges(nz):
            for name, call, want in (("mgk_jacobi_range_f32", lambda o: L.mgk_jacobi_range_f32(mgk.ctx, g32p, coef, dinv, scale, db32, du32, o, z0, z1, None), j32),
                                     ("mgk_residual_range_f32", lambda o: L.mgk_residual_range_f32(mgk.ctx, g32p, coef, db32, du32, o, z0, z1, None), r32),
                                     ("mgk_prolong_jacobi_range_f32",
                                      lambda o: L.mgk_prolong_jacobi_range_f32(mgk.ctx, g32p, gc32p, coef, dinv, scale, db32, duc32, du32, o, z0, z1, None), pj32)):
                o = mgk.to_field32(g32, fill32)
                mgk._chk(call(o))
                check(mgk.from_field32(g32, o), want, nz, z0, z1, name)
                mgk.free(o)
        for k0, k1 in _ranges(nzc):
            o = mgk.to_field32(gc32, fillc32)
            mgk._chk(L.mgk_residual_restrict_range_f32(mgk.ctx, g32p, gc32p, coef, db32, du32, o, k0, k1, None))
            check(mgk.from_field32(gc32, o), rr32, nzc, k0, k1, "mgk_residual_restrict_range_f32")
            mgk.free(o)
    assert np.array_equal(mgk.from_field(g, du), u) and np.array_equal(mgk.from_field(g, db), b)
    for p in own:
        mgk.free(p)


# ------------------------------------------------------------------------------------------------------------------------------
# the layout: mgk_pack_* / mgk_unpack_* against the numpy layout, on guarded buffers, compact arrays of distinct values
# ------------------------------------------------------------------------------------------------------------------------------
def body_layout(mgk, dim, nx, ny, nz):
    L = mgk.L
    n = nx * ny * nz
    compact = 1.0 + np.arange(n, dtype=np.float64)                 # distinct, exact in fp32 too, no zero
    for dtype, pack, unpack in ((np.float64, L.mgk_pack_f64, L.mgk_unpack_f64), (np.float32, L.mgk_pack_f32, L.mgk_unpack_f32)):
        f32 = dtype == np.float32
        if f32 and dim == 2:
            continue                                               # fp32 fields are 3-D only
        g = Geom()
        mgk._chk((L.mgk_geom_init_f32 if f32 else L.mgk_geom_init)(C.byref(g), dim, nx, ny, nz))
        want = layout(g, compact, dtype)
        dc = mgk.upload(compact)
        # pack into a poisoned field: every interior cell must be written, nothing else
        f = mgk.field32(g) if f32 else mgk.field(g)
        mgk._chk(pack(mgk.ctx, C.byref(g), dc, f, None))
        got = (mgk.from_field32 if f32 else mgk.from_field)(g, f)                       # guards and frame
        assert np.array_equal(got, compact.astype(dtype)), f"mgk_pack_{'f32' if f32 else 'f64'}: interior"
        it = np.dtype(dtype).itemsize
        raw = mgk.download(f, (g.total * it + 7) // 8).view(dtype)[:g.total]
        assert np.array_equal(raw.view(np.uint8), want.view(np.uint8)), f"mgk_pack_{'f32' if f32 else 'f64'}: the padded image differs from the numpy layout"
        # unpack a field laid out on the host into a compact buffer that holds NaN
        src = (mgk.to_field32 if f32 else mgk.to_field)(g, compact)
        out = mgk.upload(np.full(n, np.nan))
        mgk._chk(unpack(mgk.ctx, C.byref(g), src, out, None))
        assert np.array_equal(mgk.download(out, n), compact), f"mgk_unpack_{'f32' if f32 else 'f64'}"
        assert np.array_equal(mgk.download(dc, n), compact)
        for p in (dc, f, src, out):
            mgk.free(p)


# ------------------------------------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------------------------------------
CASES = [
    # ---- mgk_kernels.hip: single passes of k_stencil (tile-table indices 0 .. 2, the row form 34, the 2-D tiles at 255 / 511)
    (K.test_stencil_modes_bit_exact, (3, 7, 2), _w("mgk_jacobi_f64 mgk_residual_f64 mgk_cheby_f64")),
    (K.test_stencil_modes_bit_exact, (3, 31, 0), _w("mgk_jacobi_f64 mgk_residual_f64 mgk_cheby_f64")),
    (K.test_stencil_modes_bit_exact, (3, 127, 34), _w("mgk_jacobi_f64")),
    (K.test_stencil_modes_bit_exact, (2, 15, 1), _w("mgk_jacobi_f64 mgk_residual_f64 mgk_cheby_f64")),
    (K.test_stencil_modes_bit_exact, (2, 255, 0), _w("mgk_jacobi_f64 mgk_residual_f64 mgk_cheby_f64")),
    (K.test_stencil_modes_bit_exact, (2, 255, 1), _w("mgk_jacobi_f64 mgk_residual_f64 mgk_cheby_f64")),
    (K.test_stencil_modes_bit_exact, (2, 511, 2), _w("mgk_jacobi_f64 mgk_residual_f64 mgk_cheby_f64")),
    (DC.test_single_pass_kernels, (3, 7, ((-1, -1), (0, 5), (2, -1))), _w("mgk_apply_f64 mgk_jacobi_sumsq_f64 mgk_jacobi_range_f64 mgk_residual_range_f64 mgk_jacobi_sumsq_range_f64")),
    (DC.test_single_pass_kernels, (2, 255, ((2, -1),)), _w("mgk_apply_f64 mgk_jacobi_sumsq_f64 mgk_jacobi_range_f64 mgk_residual_range_f64 mgk_jacobi_sumsq_range_f64")),
    (K.test_zero_guess_sweep_and_sumsq, (2, 7), _w("mgk_jacobi_zero_f64")),
    (K.test_zero_guess_sweep_and_sumsq, (2, 255), _w("mgk_jacobi_zero_f64")),
    (K.test_zero_guess_sweep_and_sumsq, (3, 7), _w("mgk_jacobi_zero_f64")),
    (K.test_transfer_bit_exact, (2, 7), _w("mgk_restrict_fw_f64 mgk_prolong_add_f64")),
    (K.test_transfer_bit_exact, (2, 127), _w("mgk_restrict_fw_f64 mgk_prolong_add_f64")),
    (K.test_transfer_bit_exact, (3, 7), _w("mgk_restrict_fw_f64 mgk_prolong_add_f64")),
    (K.test_transfer_bit_exact, (3, 31), _w("mgk_restrict_fw_f64 mgk_prolong_add_f64")),
    (K.test_rhs_fill_and_error_sums, (2, 33), _w("mgk_fill_separable_f64")),
    (K.test_rhs_fill_and_error_sums, (3, 17), _w("mgk_fill_separable_f64")),
    (K.test_sweep_with_input_residual_norm_bit_exact, (3, 31, 2), _w("mgk_jacobi_sumsq_f64")),
    (K.test_sweep_with_input_residual_norm_bit_exact, (2, 127, 0), _w("mgk_jacobi_sumsq_f64")),
    (K.test_sweep_with_norm_over_plane_ranges, (31, 0), _w("mgk_jacobi_sumsq_range_f64")),
    (DK.test_sweep_over_plane_ranges, (3, 7), _w("mgk_jacobi_range_f64")),
    (DK.test_sweep_over_plane_ranges, (2, 255), _w("mgk_jacobi_range_f64")),
    # ---- 3-D fused passes, generic forms on small cubes
    (K.test_two_sweeps_in_one_pass_bit_exact, (7,), _w("mgk_jacobi2_f64")),
    (K.test_two_sweeps_in_one_pass_bit_exact, (31,), _w("mgk_jacobi2_f64")),
    (K.test_fused_prolong_jacobi_bit_exact, (7, 0), _w("mgk_prolong_jacobi_f64")),
    (K.test_fused_prolong_jacobi_bit_exact, (31, 31), _w("mgk_prolong_jacobi_f64")),
    (K.test_fused_prolong_jacobi_plane_ranges, (31, 0, (2, 30)), _w("mgk_prolong_jacobi_range_f64")),
    (K.test_fused_prolong_jacobi_plane_ranges, (31, 31, (2, 30)), _w("mgk_prolong_jacobi_range_f64")),
    (K.test_fused_residual_restrict_bit_exact, (7,), _w("mgk_residual_restrict_f64")),
    (K.test_fused_residual_restrict_bit_exact, (15,), _w("mgk_residual_restrict_f64")),
    (K.test_fused_residual_restrict_coarse_plane_ranges, (15,), _w("mgk_residual_restrict_range_f64")),
    (K.test_fused_residual_restrict_with_coarse_first_sweep, (7,), _w("mgk_residual_restrict_jz_f64")),
    (K.test_fused_residual_restrict_on_slabs_bit_exact, (15, 1), _w("mgk_restrict_finish_f64 mgk_residual_restrict_f64")),
    (K.test_fused_residual_restrict_on_slabs_single_exchange, (31, 7), _w("mgk_residual_restrict_slab_f64")),
    (K.test_fused_residual_restrict_on_slabs_single_exchange, (15, 2), _w("mgk_residual_restrict_slab_f64")),
    (DK.test_two_sweeps_on_z_slabs, (31, (0, 9, 31)), _w("mgk_jacobi2_slab_f64")),
    # ---- the full-row forms (rows of 512 / 1024) on thin grids: every fine-level pass of the default 3-D cycle
    (HW.test_sweeps_and_norms_against_the_oracle, (511, 5),
     _w("mgk_jacobi_f64 mgk_jacobi_sumsq_f64 mgk_residual_f64 mgk_jacobi2_f64 mgk_jacobi2_sumsq_f64 mgk_jacobi2_sumsq_mid_f64 mgk_jacobi2_zero_f64")),
    (HW.test_sweeps_and_norms_against_the_oracle, (1023, 3),
     _w("mgk_jacobi_f64 mgk_jacobi_sumsq_f64 mgk_residual_f64 mgk_jacobi2_f64 mgk_jacobi2_sumsq_f64 mgk_jacobi2_sumsq_mid_f64 mgk_jacobi2_zero_f64")),
    (HW.test_transfer_passes_against_the_oracle, (511, 5),
     _w("mgk_prolong_jacobi_f64 mgk_prolong_jacobi2_f64 mgk_residual_restrict_f64 mgk_residual_restrict_jz_f64 mgk_sweep_residual_restrict_f64")),
    (HW.test_transfer_passes_against_the_oracle, (1023, 3),
     _w("mgk_prolong_jacobi_f64 mgk_prolong_jacobi2_f64 mgk_residual_restrict_f64 mgk_residual_restrict_jz_f64 mgk_sweep_residual_restrict_f64")),
    (FM.test_interp_jacobi2_3d_equals_the_oracle, (511, 5), _w("mgk_interp_jacobi2_f64")),
    (FM.test_interp_jacobi2_3d_equals_the_oracle, (1023, 3), _w("mgk_interp_jacobi2_f64")),
    # ---- the four-pass and 91-byte slab forms
    (DC.test_four_pass_kernels_on_slabs, (), _w("mgk_sweep_residual_restrict_slab_f64 mgk_jacobi2_sumsq_slab_f64")),
    (DC.test_ninety_one_byte_passes_on_slabs, (), _w("mgk_prolong_jacobi2_slab_f64 mgk_jacobi2_sumsq_mid_slab_f64")),
    # ---- 2-D fused passes of mgk_kernels.hip
    (K.test_fused_prolong_jacobi_2d_bit_exact, (7, 0), _w("mgk_prolong_jacobi_f64")),
    (K.test_fused_prolong_jacobi_2d_bit_exact, (255, 1), _w("mgk_prolong_jacobi_f64")),
    (K.test_fused_prolong_jacobi_2d_bit_exact, (127, 38), _w("mgk_prolong_jacobi_f64")),
    (K.test_fused_prolong_jacobi_2d_bit_exact, (239, 38), _w("mgk_prolong_jacobi_f64")),
    (K.test_fused_prolong_jacobi_2d_bit_exact, (243, 38), _w("mgk_prolong_jacobi_f64")),
    (K.test_two_sweeps_in_one_pass_2d_bit_exact, (7,), _w("mgk_jacobi2_2d_f64")),
    (K.test_two_sweeps_in_one_pass_2d_bit_exact, (255,), _w("mgk_jacobi2_2d_f64")),
    (K.test_two_sweeps_in_one_pass_2d_bit_exact, (511,), _w("mgk_jacobi2_2d_f64")),
    (K.test_fused_residual_restrict_2d_bit_exact, (63,), _w("mgk_residual_restrict_2d_f64")),
    (K.test_fused_residual_restrict_2d_bit_exact, (255,), _w("mgk_residual_restrict_2d_f64")),
    (K.test_2d_forms_of_the_four_pass_kernels_bit_exact, (127,), _w("mgk_sweep_residual_restrict_2d_f64 mgk_jacobi2_2d_sumsq_f64")),
    (K.test_2d_forms_of_the_four_pass_kernels_bit_exact, (243,), _w("mgk_sweep_residual_restrict_2d_f64 mgk_jacobi2_2d_sumsq_f64")),
    (K.test_norm_pass_that_stores_the_residual_and_makes_the_next_sweep, (63,), _w("mgk_jacobi_sumsq_store_f64")),
    (K.test_norm_pass_that_stores_the_residual_and_makes_the_next_sweep, (255,), _w("mgk_jacobi_sumsq_store_f64")),
    # ---- row tables
    (K.test_row_table_forms_of_the_fused_2d_kernels, (63,), _w("mgk_jacobi2_2d_rowcoef_f64 mgk_jacobi_sumsq_rowcoef_f64 mgk_prolong_jacobi_rowcoef_f64 mgk_residual_restrict_2d_rowcoef_f64")),
    (K.test_row_table_forms_of_the_fused_2d_kernels, (255,), _w("mgk_jacobi2_2d_rowcoef_f64 mgk_jacobi_sumsq_rowcoef_f64 mgk_prolong_jacobi_rowcoef_f64 mgk_residual_restrict_2d_rowcoef_f64")),
    (DK.test_row_table_zero_guess_two_sweep_norm_and_sweep_restrict, (63,), _w("mgk_jacobi_zero_rowcoef_f64 mgk_jacobi2_2d_sumsq_rowcoef_f64 mgk_sweep_residual_restrict_2d_rowcoef_f64")),
    (DK.test_row_table_zero_guess_two_sweep_norm_and_sweep_restrict, (243,), _w("mgk_jacobi_zero_rowcoef_f64 mgk_jacobi2_2d_sumsq_rowcoef_f64 mgk_sweep_residual_restrict_2d_rowcoef_f64")),
    (DC.test_row_table_kernels_with_west_unlike_east, (7,), _w("mgk_cheby_rowcoef_f64 mgk_rowcoef_f64")),
    (DC.test_row_table_kernels_with_west_unlike_east, (127,), _w("mgk_cheby_rowcoef_f64 mgk_rowcoef_f64")),
    # ---- mgk_sweep3.hip: three sweeps / three Chebyshev steps per pass (one and two wave tiles, with the seam and without)
    (T3.test_three_sweeps_2d_bit_exact, (7,), _w("mgk_jacobi3_2d_f64 mgk_jacobi3_2d_sumsq_f64 mgk_jacobi3_2d_zero_f64")),
    (T3.test_three_sweeps_2d_bit_exact, (119,), _w("mgk_jacobi3_2d_f64 mgk_jacobi3_2d_sumsq_f64 mgk_jacobi3_2d_zero_f64")),
    (T3.test_three_sweeps_2d_bit_exact, (121,), _w("mgk_jacobi3_2d_f64 mgk_jacobi3_2d_sumsq_f64 mgk_jacobi3_2d_zero_f64")),
    (T3.test_three_sweeps_2d_bit_exact, (239,), _w("mgk_jacobi3_2d_f64 mgk_jacobi3_2d_sumsq_f64 mgk_jacobi3_2d_zero_f64")),
    (T3.test_three_sweeps_2d_bit_exact, (241,), _w("mgk_jacobi3_2d_f64 mgk_jacobi3_2d_sumsq_f64 mgk_jacobi3_2d_zero_f64")),
    (T3.test_prolongation_and_three_sweeps_2d_bit_exact, (239,), _w("mgk_prolong_jacobi3_2d_f64")),
    (T3.test_prolongation_and_three_sweeps_2d_bit_exact, (243,), _w("mgk_prolong_jacobi3_2d_f64")),
    (T3.test_three_sweeps_2d_on_row_tables, (63,), _w("mgk_jacobi3_2d_f64 mgk_prolong_jacobi3_2d_f64")),
    (T3.test_three_sweeps_with_stored_residual_2d, (7,), _w("mgk_jacobi3_2d_sumsq_store_f64")),
    (T3.test_three_sweeps_with_stored_residual_2d, (255,), _w("mgk_jacobi3_2d_sumsq_store_f64")),
    (T3.test_three_sweeps_3d_bit_exact, (7, 7, 7), _w("mgk_jacobi3_f64 mgk_jacobi3_sumsq_f64")),
    (T3.test_three_sweeps_3d_bit_exact, (119, 9, 11), _w("mgk_jacobi3_f64 mgk_jacobi3_sumsq_f64")),
    (T3.test_three_sweeps_3d_bit_exact, (121, 5, 7), _w("mgk_jacobi3_f64 mgk_jacobi3_sumsq_f64")),
    (FM.test_interp_jacobi3_2d_equals_the_oracle, (127,), _w("mgk_interp_jacobi3_2d_f64")),
    (CH.test_cheby3_2d_bit_exact, (7,), _w("mgk_cheby3_2d_f64 mgk_cheby3_2d_sumsq_f64 mgk_cheby3_2d_zero_f64")),
    (CH.test_cheby3_2d_bit_exact, (121,), _w("mgk_cheby3_2d_f64 mgk_cheby3_2d_sumsq_f64 mgk_cheby3_2d_zero_f64")),
    (CH.test_cheby3_2d_bit_exact, (239,), _w("mgk_cheby3_2d_f64 mgk_cheby3_2d_sumsq_f64 mgk_cheby3_2d_zero_f64")),
    (CH.test_prolongation_and_cheby3_2d_bit_exact, (119,), _w("mgk_prolong_cheby3_2d_f64")),
    (CH.test_prolongation_and_cheby3_2d_bit_exact, (239,), _w("mgk_prolong_cheby3_2d_f64")),
    (CH.test_cheby3_2d_on_row_tables, (63,), _w("mgk_cheby3_2d_f64 mgk_prolong_cheby3_2d_f64")),
    # ---- mgk_tail.hip: depths up to mgk_tail_max_n (63 in 2-D, 15 in 3-D)
    (DC.test_tail_cycle_with_a_set_per_level, (2, 63, 6, 3, 3), _w("mgk_tail_cycle_f64")),
    (DC.test_tail_cycle_with_a_set_per_level, (2, 15, 3, 2, 1), _w("mgk_tail_cycle_f64")),
    (DC.test_tail_cycle_with_a_set_per_level, (3, 15, 4, 3, 3), _w("mgk_tail_cycle_f64")),
    (DC.test_tail_cycle_with_a_set_per_level, (3, 7, 2, 1, 4), _w("mgk_tail_cycle_f64")),
    (K.test_lds_tail_kernel_on_row_tables, (63, 5), _w("mgk_tail_cycle_rowcoef_f64")),
    (K.test_lds_tail_kernel_on_row_tables, (7, 2), _w("mgk_tail_cycle_rowcoef_f64")),
    (DK.test_tail_cycle_with_coarse_scale_bit_exact, (63, 6, 3, 1, 0.8, 1.0, "coef7"), _w("mgk_tail_cycle_cs_f64")),
    (DK.test_tail_cycle_with_coarse_scale_bit_exact, (63, 5, 3, 3, 0.8, 0.5, "rowtab"), _w("mgk_tail_cycle_cs_f64")),
    (DK.test_tail_cycle_with_coarse_scale_bit_exact, (1, 1, 2, 1, 0.8, 1.0, "coef7"), _w("mgk_tail_cycle_cs_f64")),
    (DK.test_tail_cycle_f32_bit_exact, (15, 4, 3, 3), _w("mgk_tail_cycle_f32")),
    (DK.test_tail_cycle_f32_bit_exact, (3, 1, 0, 2), _w("mgk_tail_cycle_f32")),
    (FM.test_tail_fmg_equals_the_restatement, (2, 63, 6, 1), _w("mgk_tail_fmg_f64")),
    (FM.test_tail_fmg_equals_the_restatement, (3, 15, 4, 2), _w("mgk_tail_fmg_f64")),
    (CH.test_cheby_tail_kernel_bit_exact, (2, 63, 6, (3, 3)), _w("mgk_tail_cycle_cheby_f64")),
    (CH.test_cheby_tail_kernel_bit_exact, (3, 15, 4, (2, 1)), _w("mgk_tail_cycle_cheby_f64")),
    (CH.test_cheby_tail_kernel_bit_exact, (2, 7, 2, (0, 0)), _w("mgk_tail_cycle_cheby_f64")),
    (CH.test_cheby_tail_kernel_on_row_tables, (63, 6, (1, 4)), _w("mgk_tail_cycle_cheby_f64")),
    # ---- mgk_krylov.hip
    (GM.test_orthogonalisation_passes, (2, 127, 1, 7, 0), _w("mgk_multi_dot_f64 mgk_multi_axpy_sumsq_f64")),
    (GM.test_orthogonalisation_passes, (2, 127, 1, 7, 1), _w("mgk_multi_dot_f64 mgk_multi_axpy_sumsq_f64")),
    (GM.test_orthogonalisation_passes, (3, 31, 31, 31, 0), _w("mgk_multi_dot_f64 mgk_multi_axpy_sumsq_f64")),
    (GM.test_lincomb_and_scale_to, (2, 127, 1, 7, 0), _w("mgk_lincomb_f64 mgk_scale_to_f64")),
    (GM.test_lincomb_and_scale_to, (3, 31, 31, 31, 1), _w("mgk_lincomb_f64 mgk_scale_to_f64")),
    # ---- the flat BLAS-1 kernels, CSR, the dense coarse solve, the coupled level operator
    (DK.test_flat_kernels_bit_exact, (1,), _w("mgk_flat_axpy mgk_flat_aypx mgk_flat_axpbypcz mgk_flat_fill mgk_flat_scale mgk_flat_pointwise_mult")),
    (DK.test_flat_kernels_bit_exact, (257,), _w("mgk_flat_axpy mgk_flat_aypx mgk_flat_axpbypcz mgk_flat_fill mgk_flat_scale mgk_flat_pointwise_mult")),
    (DK.test_flat_kernels_bit_exact, (DK.CAP + 1,), _w("mgk_flat_axpy mgk_flat_aypx mgk_flat_axpbypcz mgk_flat_fill mgk_flat_scale mgk_flat_pointwise_mult")),
    (DK.test_csr_mult_bit_exact, (65, False), _w("mgk_csr_mult_f64")),
    (DK.test_csr_mult_bit_exact, (65, True), _w("mgk_csr_mult_f64")),
    (DK.test_csr_mult_into_a_padded_grid_field, (63,), _w("mgk_csr_mult_f64")),
    (DK.test_dense_mult_error_bound_and_reproducibility, (5,), _w("mgk_dense_mult_f64")),
    (DK.test_dense_mult_error_bound_and_reproducibility, (63,), _w("mgk_dense_mult_f64")),
    (DK.test_apply_add_bit_exact, (7,), _w("mgk_apply_add_f64")),
    (DK.test_apply_add_bit_exact, (255,), _w("mgk_apply_add_f64")),
    (DK.test_window_add_bit_exact, (2, 5), _w("mgk_window_add_f64")),
    (DK.test_window_add_bit_exact, (4, 3), _w("mgk_window_add_f64")),
    # ---- fp32 and the bridges
    (MX.test_fp32_kernels_bit_exact, (7,), _w("mgk_jacobi_f32 mgk_residual_f32 mgk_jacobi_zero_f32 mgk_restrict_fw_f32 mgk_prolong_add_f32")),
    (MX.test_fp32_kernels_bit_exact, (31,), _w("mgk_jacobi_f32 mgk_residual_f32 mgk_jacobi_zero_f32 mgk_restrict_fw_f32 mgk_prolong_add_f32")),
    (MX.test_two_fp32_sweeps_in_one_pass_bit_exact, (31,), _w("mgk_jacobi2_f32")),
    (MX.test_fused_residual_restrict_fp32_bit_exact, (31,), _w("mgk_residual_restrict_f32")),
    (MX.test_bridges_fp64_fp32, (7,), _w("mgk_residual_f64_to_f32 mgk_correct_f64_from_f32")),
    (MX.test_fused_correction_and_residual_bit_exact, (31, 2), _w("mgk_correct_residual_f64_f32")),
    (MW.test_sweeps_at_width, (255, 255, 5), _w("mgk_jacobi_f32 mgk_residual_f32 mgk_jacobi2_f32 mgk_jacobi2_zero_f32")),
    (MW.test_transfers_at_width, (255, 255, 5), _w("mgk_prolong_jacobi_f32 mgk_residual_restrict_f32 mgk_residual_restrict_jz_f32")),
    (MW.test_bridges_at_width, (255, 5),
     _w("mgk_residual_f64_to_f32 mgk_residual_f64_to_f32_jz mgk_correct_residual_f64_f32 mgk_correct_residual_f64_f32_jz mgk_correct_f64_from_f32")),
    (MW.test_fp32_slab_forms, (255, 13, (0, 2, 6)),
     _w("mgk_jacobi_range_f32 mgk_residual_range_f32 mgk_jacobi2_slab_f32 mgk_prolong_jacobi_range_f32 mgk_residual_restrict_slab_f32 "
        "mgk_residual_restrict_range_f32 mgk_restrict_finish_f32")),
    # ---- written here
    (body_range_forms, (3, 31, 31), _w("mgk_jacobi_range_f64 mgk_jacobi_range_f32 mgk_residual_range_f64 mgk_residual_range_f32 mgk_jacobi_sumsq_range_f64 "
                                       "mgk_prolong_jacobi_range_f64 mgk_prolong_jacobi_range_f32 mgk_residual_restrict_range_f64 mgk_residual_restrict_range_f32")),
    (body_range_forms, (3, 127, 9), _w("mgk_jacobi_range_f64 mgk_jacobi_range_f32 mgk_residual_range_f64 mgk_residual_range_f32 mgk_jacobi_sumsq_range_f64 "
                                       "mgk_prolong_jacobi_range_f64 mgk_prolong_jacobi_range_f32 mgk_residual_restrict_range_f64 mgk_residual_restrict_range_f32")),
    (body_range_forms, (2, 255, 1), _w("mgk_jacobi_range_f64 mgk_residual_range_f64 mgk_jacobi_sumsq_range_f64")),
    (body_layout, (2, 1, 1, 1), _w("mgk_pack_f64 mgk_unpack_f64")),
    (body_layout, (2, 5, 121, 1), _w("mgk_pack_f64 mgk_unpack_f64")),
    (body_layout, (2, 255, 3, 1), _w("mgk_pack_f64 mgk_unpack_f64")),
    (body_layout, (3, 7, 3, 2), _w("mgk_pack_f64 mgk_unpack_f64 mgk_pack_f32 mgk_unpack_f32")),
    (body_layout, (3, 127, 5, 3), _w("mgk_pack_f64 mgk_unpack_f64 mgk_pack_f32 mgk_unpack_f32")),
]

# bodies without a field(g) / field32(g) output, and what they do instead (the relaxed frame rule of run_case is for these alone)
_OUT = "its own output object: an uploaded image filled with a sentinel, with a sentinel tail past the field's end, compared whole"
_RAW = "uploads raw padded images with its own sentinel frame and compares every byte of the downloaded allocation"
OWN_FRAMES = {
    DK.test_flat_kernels_bit_exact: "flat arrays with sentinel doubles past n, compared bitwise",
    DK.test_csr_mult_bit_exact: "compact arrays with sentinels past the rows",
    DK.test_csr_mult_into_a_padded_grid_field: _RAW,
    DK.test_dense_mult_error_bound_and_reproducibility: "compact vectors",
    DK.test_apply_add_bit_exact: _RAW,
    DK.test_window_add_bit_exact: _RAW,
    FM.test_interp_jacobi2_3d_equals_the_oracle: _OUT, FM.test_interp_jacobi3_2d_equals_the_oracle: _OUT, FM.test_tail_fmg_equals_the_restatement: _OUT,
    GM.test_lincomb_and_scale_to: _OUT,
}
# entry points of which no call can be handed a poisoned output, with the reason
_INOUT = "its field argument is input and output at once: it comes from to_field, and what the call adds to is compared"
IN_PLACE = {
    "mgk_prolong_add_f64": _INOUT, "mgk_prolong_add_f32": _INOUT, "mgk_correct_f64_from_f32": _INOUT, "mgk_multi_axpy_sumsq_f64": _INOUT,
    "mgk_restrict_finish_f64": "adds the dk = 2 terms to the partial plane that mgk_residual_restrict_* left in bc",
    "mgk_restrict_finish_f32": "adds the dk = 2 terms to the partial plane that mgk_residual_restrict_* left in bc",
    "mgk_multi_dot_f64": "out_dev is an array of k dot products, not a field; the body compares all of them",
    "mgk_unpack_f64": "its output is a compact array, not a field; body_layout fills it with NaN itself",
    "mgk_unpack_f32": "its output is a compact array, not a field; body_layout fills it with NaN itself",
}
# bodies whose outputs hold a finite sentinel by design instead of the poison
OWN_FILL = {}
# bodies that run with the poison off, with the reason (at most three)
_UC0 = ("asserts that uc0, which no call writes when NULL is passed for it, still holds the zeros of the body's own mgk_memset0; "
        "under the poison that memset is undone")
UNPOISONED = {
    "dropin_kernels.row_table_zero_guess_two_sweep_norm_and_sweep_restrict-63": _UC0,
    "dropin_kernels.row_table_zero_guess_two_sweep_norm_and_sweep_restrict-243": _UC0,
}


def field_writers():
    """entry points of include/mgk.h with a non-const double * / float * parameter whose name does not end in _host"""
    with open(os.path.join(ROOT, "include", "mgk.h")) as fh:
        h = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    out = []
    for name, params in re.findall(r"^\s*(?:const\s+)?\w+\s*\**\s*(mgk_\w+)\s*\(([^;{]*?)\)\s*;", h, re.M | re.S):
        for p in params.split(","):
            m = re.match(r"^(const\s+)?(double|float)\s*\*\s*(\w+)$", " ".join(p.split()))
            if m and not m.group(1) and not m.group(3).endswith("_host"):
                out.append(name)
                break
    return out


OWN_FILL[body_range_forms] = "fills every output with the finite FILL: what lies outside the range must survive bitwise, and NaN has no single bit pattern to survive as"


def case_id(case):
    body, args = case[0], case[1]
    mod = body.__module__[5:-4] if body.__module__.startswith("test_") else "guarded"
    name = body.__name__[5:] if body.__name__.startswith("test_") else body.__name__
    return f"{mod}.{name}-{'-'.join(map(str, args))}".replace(" ", "")


def run_case(mgk, orc, body, args, covers, have=None):
    """body(Guarded(mgk), orc, *args) and what the module asks of every case.  have: the entry points the library exports (None: all)"""
    lacking = sorted(c for c in covers if have is not None and c not in have)
    if lacking:
        pytest.skip(f"the stand-in library lacks {lacking[0]}")
    G = Guarded(mgk, poison=case_id((body, args)) not in UNPOISONED)
    G.watch = covers
    try:
        if "orc" in inspect.signature(body).parameters:
            body(G, orc, *args)
        else:
            body(G, *args)
        called = set(G.calls)
        assert covers <= called, f"the case is there for {sorted(covers - called)}, which the body never called"
        G.assert_no_leaks()
        if G.poison:                                   # every reducing call of the body found the whole reduction scratch poisoned (the later ranges of a group excepted)
            dry = sorted(r for r in called & set(REDUCERS) if not G.scratch_poisoned_calls.get(r))
            assert not dry, f"the reduction scratch was not poisoned before any call of {dry}"
        if body in OWN_FRAMES:
            # no field(g) output to poison or to frame-check: the body lays its own sentinels around compact or raw images and compares every
            # byte of the whole allocation, which the proxy hands it after the guard check
            assert G.frame_checks + G.whole_downloads >= 1, "no frame check ran"
        else:
            assert G.frame_checks >= 1, "no frame check ran"
            if G.poison and body not in OWN_FILL:
                dry = sorted(c for c in covers if c not in IN_PLACE and not G.poisoned_calls.get(c))
                assert not dry, f"no call of {dry} was handed an output that still held the poison"
    finally:
        G.release()
        mgk.L.mgk_set_tuning(-1, -1)
    return G


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_body_on_guarded_poisoned_buffers(mgk, orc, case):
    run_case(mgk, orc, *case[:3])
