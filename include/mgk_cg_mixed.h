/* mgk_cg_mixed.h -- the three passes that join the fp64 recurrence of conjugate gradients to an fp32 preconditioner: the fp32 V-cycle of the
 * mixed-precision solver (csrc/mgk_cg_mixed.hip; host side csrc/mg_cg_mixed.c).
 * Conventions of include/mgk_cg.h, 3-D only (a 2-D geometry: MGK_EINVAL): fp64 fields in the padded level layout of g, fp32 fields in that of
 * g32 (mgk_geom_init_f32; the same nx, ny, nz), as in mgk_correct_residual_f64_f32.  The ghost ring of an input is read as what it holds, which
 * is zero; only interior points are summed and stored; no FMA, every product and sum rounded separately, A in the canonical order with
 * coef[7] = {k-1, i-1, j-1, C, j+1, i+1, k+1}.  (double) of an fp32 value is exact, (float) rounds to nearest.  Stores by field size,
 * mgk_set_tuning(variant = 0 / 1) forces ordinary / non-temporal ones.
 * Reductions: one partial per block in the caller's mgk_cg_ws, added up in a fixed order by one block -- no floating-point atomics, the same
 * bits on every run; the context's shared reduction scratch is not used.  A launcher refuses a launch of more blocks than the workspace has
 * slots, any call on a stream that is being captured, and aliased fields.  A *_host argument that is not NULL synchronises the stream and
 * returns the sum; NULL: the value stays in the workspace. */
#ifndef MGK_CG_MIXED_H
#define MGK_CG_MIXED_H
#include "mgk_cg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* sum r * (double) z32 in one pass of 12 B per unknown */
int  mgk_cg_dot_f64_f32(mgk_ctx *ctx, const mgk_geom *g, const mgk_geom *g32, const double *r, const float *z32, mgk_cg_ws *ws,
                        double *dot_host, void *stream);
/* mgk_cg_direction_apply_dot_f64 with z read in fp32: p_new = (double) z32 + beta * p_old, q = A p_new and sigma = p_new . q in ONE pass of
 * 28 B per unknown.  p_old == NULL is the first step: p_new = (double) z32, beta and p_old are not read (20 B).  The halo values of p_new
 * are recomputed from z32 and p_old.  p_new must differ from p_old, q from p_old and p_new, and neither may be z32 (MGK_EINVAL). */
int  mgk_cg_direction_apply_dot_zf32_f64(mgk_ctx *ctx, const mgk_geom *g, const mgk_geom *g32, const double *coef, double beta, const float *z32,
                                         const double *p_old, double *p_new, double *q, mgk_cg_ws *ws, double *sigma_host, void *stream);
/* x += alpha * p, r -= alpha * q, the sum of r^2 of the new r, and r32 = (float) of the new r stored in the fp32 layout: one pass of 52 B per
 * unknown.  e0 != NULL: also e0 = scale32 * (r32 * dinv32) in fp32 with dinv32 = (float) dinv, scale32 = (float) scale -- the first sweep of
 * an fp32 cycle from its zero guess, the arithmetic and the arguments of mgk_residual_f64_to_f32_jz (56 B).  p, q, x, r are four different
 * fields, r32 and e0 two more (MGK_EINVAL). */
int  mgk_cg_update_sumsq_f64_f32(mgk_ctx *ctx, const mgk_geom *g, const mgk_geom *g32, double alpha, const double *p, const double *q, double *x,
                                 double *r, float *r32, float *e0, double dinv, double scale, mgk_cg_ws *ws, double *sumsq_host, void *stream);

#ifdef __cplusplus
}
#endif
#endif
