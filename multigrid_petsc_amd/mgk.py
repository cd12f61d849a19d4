"""ctypes binding of include/mgk.h (kernel-level C ABI).  Test/bench plumbing only."""
import contextlib
import ctypes as C
import enum
import numpy as np
from ._lib import load_mgk

c_dp = C.POINTER(C.c_double)


class Geom(C.Structure):
    _fields_ = [("dim", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("pitch", C.c_int), ("plane", C.c_long), ("org", C.c_long), ("total", C.c_long)]


class MgkError(RuntimeError):
    pass


class Tune(enum.IntEnum):
    """enum mgk_tune of include/mgk.h (tests/test_abi.py holds the two together): the named values of mgk_set_tuning's first argument.
    Values below 30 that are tile-table indices or the ring / register choice of jacobi2 stay plain integers (the table in the header)."""
    DEFAULT = -1
    STORE_PLAIN = 0
    STORE_NT = 1
    LDS_TILE = 30
    ROW = 31
    ROW_PD2 = 32
    ROW_UNCOND = 33
    ROW_DPP = 34
    ROW_PRED_DPP = 35
    J2_REG_PRED = 36
    J2_RING_PRED = 37
    PJ2D_WAVES = 38
    J2_RING_OLD = 39
    SRR_TY2 = 40
    SRR_TY4 = 41
    J2_ZERO_RINGB = 45
    PJ2_COPY = 46
    J3_2D_MARCH = 50
    J3_2D_CHUNK4 = 51
    J3_2D_CHUNK8 = 52
    DISPATCH_ORDER = 53
    XCD_ORDER = 54
    RR2D_MARCH = 55
    RR2D_SHORT = 56
    RESERVED_57 = 57
    J3_2D_ODD_DOWN = 58
    J3_2D_ALL_DOWN = 59
    J3_2D_STORE_PLAIN = 60
    J3_2D_STORE_NT = 61
    J3_3D_TY2 = 62
    J3_3D_TY3 = 63
    J3_3D_ROWWISE = 64
    NO_EXACT_FMA = 65
    J3_3D_WAVES = 66
    J3_3D_STACKED = 67
    J3_3D_STACKED_DISPATCH = 68
    NO_PROLONG_TRIPLE = 69


# MGK_TUNE_J3S_NORM_R3 of include/mgk.h: the next value, beside the enum there and here (the enumerators mirror the C enum one to one)
TUNE_J3S_NORM_R3 = 70
# MGK_TUNE_J3S_B_NT: the stacked 3-D three-sweep pass loads b non-temporally, as it did before plain loads became its default
TUNE_J3S_B_NT = 71


@contextlib.contextmanager
def tuning(variant=-1, zchunk=-1):
    """set the calling thread's tuning knobs for the body and put (-1, -1) back on the way out, exceptions included"""
    L = load_mgk()
    L.mgk_set_tuning.restype, L.mgk_set_tuning.argtypes = None, [C.c_int, C.c_int]
    L.mgk_set_tuning(int(variant), int(zchunk))
    try:
        yield
    finally:
        L.mgk_set_tuning(-1, -1)


def _sigs(L):
    vp, i, d, sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
    G = C.POINTER(Geom)
    S = {
        "mgk_geom_init": (i, [G, i, i, i, i]),
        "mgk_device_count": (i, []),
        "mgk_set_device": (i, [i]),
        "mgk_ctx_create": (i, [C.POINTER(vp), i]),
        "mgk_ctx_destroy": (None, [vp]),
        "mgk_last_error": (C.c_char_p, []),
        "mgk_stream_compute": (vp, [vp]),
        "mgk_stream_comm": (vp, [vp]),
        "mgk_malloc": (i, [vp, C.POINTER(vp), sz]),
        "mgk_free": (i, [vp, vp]),
        "mgk_memset0": (i, [vp, vp, sz, vp]),
        "mgk_h2d": (i, [vp, vp, vp, sz]),
        "mgk_d2h": (i, [vp, vp, vp, sz]),
        "mgk_d2d": (i, [vp, vp, vp, sz, vp]),
        "mgk_sync": (i, [vp, vp]),
        "mgk_timer_create": (i, [vp, C.POINTER(vp)]),
        "mgk_timer_start": (i, [vp, vp, vp]),
        "mgk_timer_stop": (i, [vp, vp, vp]),
        "mgk_timer_elapsed_ms": (i, [vp, vp, C.POINTER(d)]),
        "mgk_timer_destroy": (None, [vp, vp]),
        "mgk_stream_wait": (i, [vp, vp, vp]),
        "mgk_pack_f64": (i, [vp, G, vp, vp, vp]),
        "mgk_unpack_f64": (i, [vp, G, vp, vp, vp]),
        "mgk_jacobi_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp]),
        "mgk_jacobi_zero_f64": (i, [vp, G, d, d, vp, vp, vp]),
        "mgk_cheby_f64": (i, [vp, G, c_dp, d, d, d, d, vp, vp, vp, vp, vp]),
        "mgk_residual_f64": (i, [vp, G, c_dp, vp, vp, vp, vp]),
        "mgk_residual_sumsq_f64": (i, [vp, G, c_dp, vp, vp, C.POINTER(d), vp]),
        "mgk_jacobi2_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp]),
        "mgk_jacobi2_f32": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp]),
        "mgk_jacobi2_2d_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp]),
        "mgk_jacobi2_2d_rowcoef_f64": (i, [vp, G, vp, vp, d, vp, vp, vp, vp]),
        "mgk_jacobi_sumsq_rowcoef_f64": (i, [vp, G, vp, vp, d, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_jacobi_sumsq_store_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_apply_add_f64": (i, [vp, G, c_dp, vp, vp, vp]),
        "mgk_window_add_f64": (i, [vp, G, G, i, vp, vp, vp, vp]),
        "mgk_dense_mult_f64": (i, [vp, i, i, vp, vp, vp, vp]),
        "mgk_residual_sumsq_rowcoef_f64": (i, [vp, G, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_prolong_jacobi_rowcoef_f64": (i, [vp, G, G, vp, vp, d, vp, vp, vp, vp, vp]),
        "mgk_residual_restrict_2d_rowcoef_f64": (i, [vp, G, G, vp, vp, vp, vp, vp, vp, d, vp]),
        "mgk_jacobi2_2d_sumsq_rowcoef_f64": (i, [vp, G, vp, vp, d, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_sweep_residual_restrict_2d_rowcoef_f64": (i, [vp, G, G, vp, vp, d, vp, vp, vp, vp, vp, vp, d, vp]),
        "mgk_tail_cycle_rowcoef_f64": (i, [vp, G, i, C.POINTER(i), C.POINTER(vp), C.POINTER(vp), d, i, i, vp, vp, vp]),
        "mgk_jacobi_sumsq_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_restrict_fw_f64": (i, [vp, G, G, vp, vp, vp]),
        "mgk_prolong_add_f64": (i, [vp, G, G, vp, vp, vp]),
        "mgk_sumsq_f64": (i, [vp, G, vp, C.POINTER(d), vp]),
        "mgk_fill_separable_f64": (i, [vp, G, vp, vp, vp, vp, vp]),
        "mgk_error_sums_f64": (i, [vp, G, vp, vp, vp, vp, c_dp, vp]),
        "mgk_set_tuning": (None, [i, i]),
        "mgk_geom_init_f32": (i, [G, i, i, i, i]),
        "mgk_jacobi_f32": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp]),
        "mgk_jacobi_range_f32": (i, [vp, G, c_dp, d, d, vp, vp, vp, i, i, vp]),
        "mgk_jacobi2_slab_f32": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, i, i, i, i, vp]),
        "mgk_jacobi_zero_f32": (i, [vp, G, d, d, vp, vp, vp]),
        "mgk_residual_f32": (i, [vp, G, c_dp, vp, vp, vp, vp]),
        "mgk_restrict_fw_f32": (i, [vp, G, G, vp, vp, vp]),
        "mgk_prolong_add_f32": (i, [vp, G, G, vp, vp, vp]),
        "mgk_residual_f64_to_f32": (i, [vp, G, G, c_dp, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_correct_f64_from_f32": (i, [vp, G, G, vp, vp, vp]),
        "mgk_correct_residual_f64_f32": (i, [vp, G, G, c_dp, vp, vp, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_pack_f32": (i, [vp, G, vp, vp, vp]),
        "mgk_unpack_f32": (i, [vp, G, vp, vp, vp]),
        "mgk_apply_f64": (i, [vp, G, c_dp, vp, vp, vp]),
        "mgk_residual_restrict_f64": (i, [vp, G, G, c_dp, vp, vp, vp, vp]),
        "mgk_residual_restrict_f32": (i, [vp, G, G, c_dp, vp, vp, vp, vp]),
        "mgk_residual_restrict_jz_f64": (i, [vp, G, G, c_dp, vp, vp, vp, vp, d, d, vp]),
        "mgk_residual_restrict_jz_f32": (i, [vp, G, G, c_dp, vp, vp, vp, vp, d, d, vp]),
        "mgk_residual_range_f64": (i, [vp, G, c_dp, vp, vp, vp, i, i, vp]),
        "mgk_residual_range_f32": (i, [vp, G, c_dp, vp, vp, vp, i, i, vp]),
        "mgk_restrict_finish_f64": (i, [vp, G, G, vp, vp, vp]),
        "mgk_restrict_finish_f32": (i, [vp, G, G, vp, vp, vp]),
        "mgk_flat_dot": (i, [vp, C.c_long, vp, vp, C.POINTER(d), vp]),
        "mgk_stream_triad_f64": (i, [vp, C.c_long, vp, vp, vp, d, i, i, vp]),
        "mgk_flat_axpy": (i, [vp, C.c_long, d, vp, vp, vp]),
        "mgk_flat_scale": (i, [vp, C.c_long, d, vp, vp]),
        "mgk_flat_fill": (i, [vp, C.c_long, d, vp, vp]),
        "mgk_flat_aypx": (i, [vp, C.c_long, d, vp, vp, vp]),
        "mgk_flat_axpbypcz": (i, [vp, C.c_long, d, d, d, vp, vp, vp, vp]),
        "mgk_flat_pointwise_mult": (i, [vp, C.c_long, vp, vp, vp, vp]),
        "mgk_defer_result": (i, [vp, vp]),
        "mgk_csr_mult_f64": (i, [vp, C.c_long, vp, vp, vp, vp, vp, d, vp, i, C.c_long, C.c_long, vp]),
        "mgk_jacobi_zero_rowcoef_f64": (i, [vp, G, vp, d, vp, vp, vp]),
        "mgk_rowcoef_f64": (i, [vp, G, i, vp, vp, d, vp, vp, vp, vp]),
        "mgk_cheby_rowcoef_f64": (i, [vp, G, vp, vp, d, d, d, vp, vp, vp, vp, vp]),
        "mgk_jacobi_range_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, i, i, vp]),
        "mgk_jacobi2_slab_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, i, i, i, i, vp]),
        "mgk_prolong_jacobi_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, vp]),
        "mgk_prolong_jacobi_f32": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, vp]),
        "mgk_prolong_jacobi_range_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, i, i, vp]),
        "mgk_prolong_jacobi_range_f32": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, i, i, vp]),
        "mgk_residual_restrict_range_f64": (i, [vp, G, G, c_dp, vp, vp, vp, i, i, vp]),
        "mgk_residual_restrict_range_f32": (i, [vp, G, G, c_dp, vp, vp, vp, i, i, vp]),
        "mgk_residual_restrict_slab_f64": (i, [vp, G, G, G, c_dp, vp, vp, vp, i, vp, i, i, vp]),
        "mgk_residual_restrict_slab_f32": (i, [vp, G, G, G, c_dp, vp, vp, vp, i, vp, i, i, vp]),
        "mgk_residual_restrict_2d_f64": (i, [vp, G, G, c_dp, vp, vp, vp, vp, d, d, vp]),
        "mgk_sweep_residual_restrict_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, vp, d, d, vp]),
        "mgk_sweep_residual_restrict_ok_f64": (i, [G, G]),
        "mgk_jacobi2_sumsq_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_jacobi2_sumsq_ok_f64": (i, [G]),
        "mgk_jacobi2_sumsq_mid_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_prolong_jacobi2_ok_f64": (i, [G, G]),
        "mgk_prolong_jacobi2_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, vp]),
        "mgk_jacobi2_zero_ok_f64": (i, [G]),
        "mgk_jacobi2_zero_ok_f32": (i, [G]),
        "mgk_jacobi2_zero_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp]),
        "mgk_jacobi2_zero_f32": (i, [vp, G, c_dp, d, d, vp, vp, vp]),
        "mgk_jacobi2_2d_sumsq_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_jacobi3_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp]),
        "mgk_jacobi3_sumsq_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_jacobi3_sumsq_mid_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_jacobi3_mid_ok_f64": (i, [G]),
        "mgk_prolong_jacobi3_ok_f64": (i, [G, G]),
        "mgk_prolong_jacobi3_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, vp]),
        "mgk_jacobi3_2d_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp, vp, vp]),
        "mgk_jacobi3_2d_sumsq_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_jacobi3_2d_zero_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp, vp]),
        "mgk_jacobi3_2d_sumsq_store_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_prolong_jacobi3_2d_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, vp, vp, vp]),
        # KSPCHEBYSHEV with max_it = 3 in one pass: cheb = 7 doubles {s, (c_km1, c_k, c_z) of step 2, of step 3} in place of scale
        "mgk_cheby3_2d_f64": (i, [vp, G, c_dp, d, c_dp, vp, vp, vp, vp, vp, vp]),
        "mgk_cheby3_2d_sumsq_f64": (i, [vp, G, c_dp, d, c_dp, vp, vp, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_cheby3_2d_zero_f64": (i, [vp, G, c_dp, d, c_dp, vp, vp, vp, vp, vp]),
        "mgk_prolong_cheby3_2d_f64": (i, [vp, G, G, c_dp, d, c_dp, vp, vp, vp, vp, vp, vp, vp]),
        "mgk_tail_cycle_cheby_f64": (i, [vp, G, i, C.POINTER(i), c_dp, c_dp, C.POINTER(vp), C.POINTER(vp), d, d, i, i, vp, vp, vp]),
        "mgk_sweep_residual_restrict_2d_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, vp, d, d, vp]),
        "mgk_jacobi2_sumsq_slab_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, i, i, i, i, i, C.POINTER(i), vp]),
        "mgk_jacobi2_sumsq_mid_slab_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp, i, i, i, i, i, C.POINTER(i), vp]),
        "mgk_prolong_jacobi2_slab_ok_f64": (i, [G, G, i]),
        "mgk_prolong_jacobi2_slab_f64": (i, [vp, G, G, G, G, c_dp, d, d, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]),
        "mgk_sweep_residual_restrict_slab_ok_f64": (i, [G, G]),
        "mgk_sweep_residual_restrict_slab_f64": (i, [vp, G, G, G, c_dp, d, d, vp, vp, vp, vp, vp, vp, i, i, vp, i, i, vp]),
        "mgk_ctx_set_chunk_planes": (i, [vp, i]),
        "mgk_residual_f64_to_f32_jz": (i, [vp, G, G, c_dp, vp, vp, vp, vp, d, d, C.POINTER(d), vp]),
        "mgk_correct_residual_f64_f32_jz": (i, [vp, G, G, c_dp, vp, vp, vp, vp, vp, vp, d, d, C.POINTER(d), vp]),
        "mgk_tail_cycle_f64": (i, [vp, G, i, C.POINTER(i), c_dp, c_dp, d, i, i, vp, vp, vp]),
        "mgk_tail_fmg_f64": (i, [vp, G, i, C.POINTER(i), c_dp, c_dp, d, i, i, i, vp, vp, vp]),
        "mgk_interp_jacobi2_ok_f64": (i, [G, G]),
        "mgk_interp_jacobi2_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp]),
        "mgk_interp_jacobi3_2d_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, vp, vp]),
        "mgk_tail_cycle_cs_f64": (i, [vp, G, i, C.POINTER(i), c_dp, c_dp, C.POINTER(vp), C.POINTER(vp), d, d, i, i, vp, vp, vp]),
        "mgk_tail_cycle_f32": (i, [vp, G, i, C.POINTER(i), c_dp, c_dp, d, i, i, vp, vp, vp]),
        "mgk_tail_max_n": (i, [i]),
        "mgk_debug_tail_stamps": (None, [vp]),
        "mgk_debug_partials": (vp, [vp, C.POINTER(C.c_long)]),
        "mgk_debug_set_max_partials": (i, [vp, i]),
        "mgk_jacobi_sumsq_range_f64": (i, [vp, G, c_dp, d, d, vp, vp, vp, i, i, i, C.POINTER(i), vp]),
        "mgk_partials_finish": (i, [vp, i, C.POINTER(d), vp]),
        "mgk_host_alloc": (i, [vp, C.POINTER(vp), sz]),
        "mgk_host_free": (i, [vp, vp]),
        "mgk_d2h_async": (i, [vp, vp, vp, sz, vp]),
        "mgk_h2d_async": (i, [vp, vp, vp, sz, vp]),
        "mgk_delay_us": (i, [vp, d, vp]),
        # Krylov orthogonalisation: v = array of k device pointers
        "mgk_multi_dot_f64": (i, [vp, G, i, C.POINTER(vp), vp, vp, c_dp, vp]),
        "mgk_multi_axpy_sumsq_f64": (i, [vp, G, i, vp, C.POINTER(vp), vp, C.POINTER(d), vp]),
        "mgk_krylov_fetch": (i, [vp, i, c_dp, C.POINTER(d), vp]),
        "mgk_lincomb_f64": (i, [vp, G, i, c_dp, C.POINTER(vp), vp, vp]),
        "mgk_scale_to_f64": (i, [vp, G, d, vp, vp, vp, vp]),
        "mgk_paced_copy": (i, [vp, vp, vp, sz, d, i, vp]),
        # y-line Jacobi: (ctab, ltab, gtab, b, u or None, z) / (qtab, scale, z, u or None, unew)
        "mgk_line_forward_f64": (i, [vp, G, vp, vp, vp, vp, vp, vp, vp]),
        "mgk_line_backward_f64": (i, [vp, G, vp, d, vp, vp, vp, vp]),
        # x-line Jacobi: (ctab, gtab, gstride, b, u or None, z) / (ctab, gtab, gstride, scale, z, u or None, unew)
        "mgk_xline_forward_f64": (i, [vp, G, vp, vp, C.c_long, vp, vp, vp, vp]),
        "mgk_xline_backward_f64": (i, [vp, G, vp, vp, C.c_long, d, vp, vp, vp, vp]),
        # the y-line sweep in chunks of c rows: (c, ctab, ltab, gtab, b, u or None, z) / (c, qtab, z) / (c, ctab, Ltab, Gtab, Qtab, z) /
        # (c, vtab, wtab, scale, z, u or None, unew)
        "mgk_line_chunk_forward_f64": (i, [vp, G, i, vp, vp, vp, vp, vp, vp, vp]),
        "mgk_line_chunk_backward_f64": (i, [vp, G, i, vp, vp, vp]),
        "mgk_line_chunk_reduce_f64": (i, [vp, G, i, vp, vp, vp, vp, vp, vp]),
        "mgk_line_chunk_correct_f64": (i, [vp, G, i, vp, vp, d, vp, vp, vp, vp]),
        # the x-line sweep in chunks of c columns: (c, ctab, gtab, gstride, b, u or None, t, sep) / (c, ctab, gtab, gstride, t, sep) /
        # (c, ctab, SLtab, SGtab, SQtab, sstride, sep) / (c, vtab, wtab, gstride, scale, t, sep, u or None, unew)
        "mgk_xline_chunk_forward_f64": (i, [vp, G, i, vp, vp, C.c_long, vp, vp, vp, vp, vp]),
        "mgk_xline_chunk_backward_f64": (i, [vp, G, i, vp, vp, C.c_long, vp, vp, vp]),
        "mgk_xline_chunk_reduce_f64": (i, [vp, G, i, vp, vp, vp, vp, C.c_long, vp, vp]),
        "mgk_xline_chunk_correct_f64": (i, [vp, G, i, vp, vp, C.c_long, d, vp, vp, vp, vp, vp]),
        # the LDS-resident coarse levels of a line cycle in one launch: (nlev, n, pc, ctab[], ltab[], gtab[], qtab[], xgtab[], xgs[], scale, v0, v1, b, u)
        "mgk_tail_cycle_line_f64": (i, [vp, G, i, C.POINTER(i), i, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                        C.POINTER(C.c_long), d, i, i, vp, vp, vp]),
        # red-black Gauss-Seidel: (coef, dinv, scale, ctab, dtab, nsweeps, b, u or None, unew) / (gf, gc, ..., nsweeps, b, uc, u, unew)
        "mgk_rbgs_2d_f64": (i, [vp, G, c_dp, d, d, vp, vp, i, vp, vp, vp, vp]),
        "mgk_prolong_rbgs_2d_f64": (i, [vp, G, G, c_dp, d, d, vp, vp, i, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in S.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return S


def cg_sigs(L):
    """include/mgk_cg.h: the two fused passes of the CG driver and their reduction workspace, bound on first use (the stand-in libraries of
    the host tests need not have them)"""
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    G = C.POINTER(Geom)
    S = {
        "mgk_cg_workspace_create": (i, [vp, C.POINTER(vp)]),
        "mgk_cg_workspace_destroy": (None, [vp, vp]),
        "mgk_cg_workspace_debug": (i, [vp, C.POINTER(vp), C.POINTER(i)]),
        # (coef, beta, z, p_old or None, p_new, q, ws, sigma or None) / (alpha, p, q, x, r, ws, sumsq or None)
        "mgk_cg_direction_apply_dot_f64": (i, [vp, G, c_dp, d, vp, vp, vp, vp, vp, C.POINTER(d), vp]),
        "mgk_cg_update_sumsq_f64": (i, [vp, G, d, vp, vp, vp, vp, vp, C.POINTER(d), vp]),
    }
    for name, (res, args) in S.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return S


def cg_mixed_sigs(L):
    """include/mgk_cg_mixed.h: the three passes between the fp64 CG recurrence and the fp32 cycle, bound on first use; the workspace is the one of
    cg_sigs"""
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    G = C.POINTER(Geom)
    S = {
        # (g, g32, r, z32, ws, dot or None)
        "mgk_cg_dot_f64_f32": (i, [vp, G, G, vp, vp, vp, C.POINTER(d), vp]),
        # (g, g32, coef, beta, z32, p_old or None, p_new, q, ws, sigma or None)
        "mgk_cg_direction_apply_dot_zf32_f64": (i, [vp, G, G, c_dp, d, vp, vp, vp, vp, vp, C.POINTER(d), vp]),
        # (g, g32, alpha, p, q, x, r, r32, e0 or None, dinv, scale, ws, sumsq or None)
        "mgk_cg_update_sumsq_f64_f32": (i, [vp, G, G, d, vp, vp, vp, vp, vp, vp, d, d, vp, C.POINTER(d), vp]),
    }
    cg_sigs(L)
    for name, (res, args) in S.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return S


class Mgk:
    """Thin object wrapper: one context on one device."""

    def __init__(self, device=0):
        self.L = load_mgk()
        self.symbols = _sigs(self.L)
        self.ctx = C.c_void_p()
        self._chk(self.L.mgk_ctx_create(C.byref(self.ctx), device))

    def _chk(self, rc):
        if rc != 0:
            raise MgkError(f"mgk call failed: rc={rc}: {self.L.mgk_last_error().decode()}")

    def close(self):
        if self.ctx:
            self.L.mgk_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    # -- geometry / memory --
    def geom(self, dim, nx, ny=None, nz=None):
        g = Geom()
        ny = nx if ny is None else ny
        nz = (nx if dim == 3 else 1) if nz is None else nz
        self._chk(self.L.mgk_geom_init(C.byref(g), dim, nx, ny, nz))
        return g

    def alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.L.mgk_malloc(self.ctx, C.byref(p), nbytes))
        return p

    def free(self, p):
        self._chk(self.L.mgk_free(self.ctx, p))

    def field(self, g):
        return self.alloc(8 * g.total)

    def sync(self):
        self._chk(self.L.mgk_sync(self.ctx, None))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        p = self.alloc(arr.nbytes)
        self._chk(self.L.mgk_h2d(self.ctx, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return p

    def download(self, p, n):
        out = np.empty(n, dtype=np.float64)
        self._chk(self.L.mgk_d2h(self.ctx, out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def to_field(self, g, compact):
        """compact lexicographic numpy array -> new padded device field"""
        tmp = self.upload(np.asarray(compact, dtype=np.float64).ravel())
        f = self.field(g)
        self._chk(self.L.mgk_pack_f64(self.ctx, C.byref(g), tmp, f, None))
        self.sync()
        self.free(tmp)
        return f

    def from_field(self, g, f):
        n = g.nx * g.ny * g.nz
        tmp = self.alloc(8 * n)
        self._chk(self.L.mgk_unpack_f64(self.ctx, C.byref(g), f, tmp, None))
        self.sync()
        out = self.download(tmp, n)
        self.free(tmp)
        return out

    # -- fp32 fields (mixed-precision cycle) --
    def geom32(self, n):
        g = Geom()
        self._chk(self.L.mgk_geom_init_f32(C.byref(g), 3, n, n, n))
        return g

    def field32(self, g32):
        """new zero-filled padded fp32 field"""
        return self.alloc(4 * g32.total)

    def to_field32(self, g32, compact):
        tmp = self.upload(np.asarray(compact, dtype=np.float64).ravel())
        f = self.alloc(4 * g32.total)
        self._chk(self.L.mgk_pack_f32(self.ctx, C.byref(g32), tmp, f, None))
        self.sync()
        self.free(tmp)
        return f

    def from_field32(self, g32, f):
        n = g32.nx * g32.ny * g32.nz
        tmp = self.alloc(8 * n)
        self._chk(self.L.mgk_unpack_f32(self.ctx, C.byref(g32), f, tmp, None))
        self.sync()
        out = self.download(tmp, n)
        self.free(tmp)
        return out.astype(np.float32)

    def raw_field(self, g, f):
        """whole padded allocation (ghosts included) as a flat numpy array"""
        return self.download(f, g.total)

    def tail_cycle_line(self, g0, n, pc, ctab, ltab=None, gtab=None, qtab=None, xgtab=None, xgs=None, scale=1.0, v=(3, 3), b=None, u=None):
        """mgk_tail_cycle_line_f64: the levels n[0] > n[1] > ... of a line cycle in one launch, b of the first level in, its u out (padded
        device fields of geometry g0).  pc: 1 y-line, 2 x-line, 3 alternating.  The tables are lists of device pointers, one per level
        (None: the argument is passed as NULL); xgs the row strides of the x tables.  Returns the kernel ABI's return code"""
        nl = len(n)

        def ptrs(tabs):
            return None if tabs is None else (C.c_void_p * nl)(*[t if isinstance(t, C.c_void_p) else C.c_void_p(t) for t in tabs])

        strides = None if xgs is None else (C.c_long * nl)(*xgs)
        return self.L.mgk_tail_cycle_line_f64(self.ctx, C.byref(g0), nl, (C.c_int * nl)(*n), pc, ptrs(ctab), ptrs(ltab), ptrs(gtab), ptrs(qtab),
                                              ptrs(xgtab), strides, scale, v[0], v[1], b, u, None)

    @staticmethod
    def coef(vals):
        return (C.c_double * len(vals))(*vals)
