/* mgk_sweep3.h -- the stacked three-sweep pass of the 3-D fine level (csrc/mgk_sweep3.hip, k_jacobi3s).
 * Conventions of include/mgk.h: fields are device pointers with the geometry's ghost ring and row padding; the ghost ring of u is read as
 * zeros (homogeneous Dirichlet); nothing outside the interior of unew is written (its ghost ring and padding stay what they were, the ghost
 * column next to the last interior column of an odd nx is written as zero, as by every pair-wise kernel); unew must not be u or b
 * (MGK_EINVAL); u and b are not modified.  Coefficients: coef[7] = {k-1, i-1, j-1, C, j+1, i+1, k+1}, dinv the inverse diagonal. */
#ifndef MGK_SWEEP3_H
#define MGK_SWEEP3_H
#include "mgk.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 1 if mgk_jacobi3_sumsq_mid_f64 is built for the geometry: whole 3-D grids with rows of 512 or 1024 points (nx = 511, 1023; any ny, nz) */
int  mgk_jacobi3_mid_ok_f64(const mgk_geom *g);
/* unew = J(J(J(u))) and *sumsq_host = || b - A J(u) ||^2, the residual of the FIRST sweep's output (which is not stored), in one pass of
 * 24 B per unknown: the three-sweep counterpart of mgk_jacobi2_sumsq_mid_f64.  Bit-identical to three mgk_jacobi_f64 calls; the sum is formed
 * from per-block partials in a fixed order.  Other shapes: MGK_EINVAL with a message.  The knobs of mgk_set_tuning: the chunk length in z,
 * MGK_TUNE_J3_3D_STACKED_DISPATCH (tiles in dispatch order), MGK_TUNE_J3S_B_NT (b loaded non-temporally), MGK_TUNE_NO_EXACT_FMA. */
int  mgk_jacobi3_sumsq_mid_f64(mgk_ctx *ctx, const mgk_geom *g, const double *coef, double dinv, double scale,
                               const double *b, const double *u, double *unew, double *sumsq_host, void *stream);

/* 1 if mgk_prolong_jacobi3_f64 is built for the pair of geometries: gf a whole 3-D grid with rows of 512 or 1024 points and gf = 2 gc + 1 in
 * every direction.  0 under MGK_TUNE_NO_PROLONG_TRIPLE (the entry point itself stays callable) */
int  mgk_prolong_jacobi3_ok_f64(const mgk_geom *gf, const mgk_geom *gc);
/* unew = J(J(J(u + P uc))): the prolongation, its correction and three post-smoothing sweeps in one pass of 25 B per fine unknown (u, b and
 * uc / 8 read, unew written once).  Bit-identical to mgk_prolong_jacobi_f64 followed by two mgk_jacobi_f64.  unew must not be u, b or uc;
 * u, b and uc are not modified.  Other shapes: MGK_EINVAL with a message.  Knobs: the chunk length in z, MGK_TUNE_J3_3D_STACKED_DISPATCH,
 * MGK_TUNE_J3S_B_NT, MGK_TUNE_NO_EXACT_FMA. */
int  mgk_prolong_jacobi3_f64(mgk_ctx *ctx, const mgk_geom *gf, const mgk_geom *gc, const double *coef, double dinv, double scale,
                             const double *b, const double *uc, const double *u, double *unew, void *stream);

#ifdef __cplusplus
}
#endif
#endif
