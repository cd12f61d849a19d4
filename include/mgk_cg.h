/* mgk_cg.h -- the two fused passes of V-cycle-preconditioned conjugate gradients (csrc/mgk_cg.hip; host side csrc/mg_cg.c; DESIGN.md
 * section 8l) and the reduction workspace they sum into.
 * Conventions of include/mgk.h: fp64 fields are device pointers in the padded level layout of the geometry, 2-D and 3-D; the ghost ring of an
 * input is read as what it holds, which is zero (homogeneous Dirichlet); only interior points are summed and stored -- the ghost ring and the
 * row padding of an output stay what they were; no FMA, every product and every sum rounded separately; A in the canonical order, with the
 * constant coefficients of mgk_apply_f64: coef[5] = {i-1, j-1, C, j+1, i+1} in 2-D, coef[7] = {k-1, i-1, j-1, C, j+1, i+1, k+1} in 3-D.
 * Stores by field size, mgk_set_tuning(variant = 0 / 1) forces ordinary / non-temporal ones.
 * Reductions: one partial per block in the caller's workspace, added up in a fixed order by one block -- no floating-point atomics, the same
 * bits on every run.  The context's shared reduction scratch is not used.  A launcher refuses a launch of more blocks than the workspace has
 * slots, and any call on a stream that is being captured (the reduced value is copied to the host). */
#ifndef MGK_CG_H
#define MGK_CG_H
#include "mgk.h"
#ifdef __cplusplus
extern "C" {
#endif

/* device partial slots, two device result slots (sigma, sum r^2) and their pinned landing area; owned by the caller (the CG driver) */
typedef struct mgk_cg_ws mgk_cg_ws;
int  mgk_cg_workspace_create(mgk_ctx *ctx, mgk_cg_ws **ws);
void mgk_cg_workspace_destroy(mgk_ctx *ctx, mgk_cg_ws *ws);
/* test aid: the device address of the partial slots and their number (fill and read them with mgk_h2d / mgk_d2h) */
int  mgk_cg_workspace_debug(mgk_cg_ws *ws, double **parts_dev, int *nslots);

/* p_new = z + beta * p_old, q = A p_new and sigma = p_new . q in ONE pass of 32 B per unknown (z, p_old read; p_new, q written).
 * p_old == NULL is the first step: p_new = z, beta and p_old are not read (24 B).  The halo values of p_new that a tile needs are
 * recomputed from z and p_old; the sum counts every interior point once.  p_new must differ from p_old and z, q from z, p_old and p_new
 * (MGK_EINVAL): tiles read the old halo values while their neighbours store.  sigma_host non-NULL: synchronises the stream and returns
 * the sum; NULL: the value stays in the workspace. */
int  mgk_cg_direction_apply_dot_f64(mgk_ctx *ctx, const mgk_geom *g, const double *coef, double beta, const double *z, const double *p_old,
                                    double *p_new, double *q, mgk_cg_ws *ws, double *sigma_host, void *stream);
/* x += alpha * p, r -= alpha * q and the sum of r^2 of the new r in one pass of 48 B per unknown, in place (pointwise).  p, q, x, r are
 * four different fields (MGK_EINVAL).  sumsq_host as sigma_host above. */
int  mgk_cg_update_sumsq_f64(mgk_ctx *ctx, const mgk_geom *g, double alpha, const double *p, const double *q, double *x, double *r,
                             mgk_cg_ws *ws, double *sumsq_host, void *stream);

#ifdef __cplusplus
}
#endif
#endif
