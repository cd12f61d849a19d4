/*
 * mg_triple.c -- the middle pass of the 75-byte 3-D fine level (fuse bit 16, MG_FUSE_TRIPLE_MID, include/mgsolve.h).
 * Where level 0's post-smoothing stopped one sweep short (fuse bit 12: prolongation + two sweeps in one pass), the pass that evaluates the
 * norm makes that sweep, the norm of its result and the first TWO pre-smoothing sweeps of the next cycle:
 *
 *   (P + S1, S2)  (S3, N + S1', S2')  (S3' + R)  =  25 + 24 + 26  =  75 B per fine unknown and cycle, instead of
 *   (P + S1, S2)  (S3, N + S1')  (S2', S3')  (R)  =  25 + 24 + 24 + 18  =  91 B
 *
 * u stays one sweep behind the iterate the norm belongs to (it is never stored), tmp is two sweeps ahead of it.  mg_solver.c decides WHERE the
 * pass runs (vcycle_once) and keeps the flags; this file is the only host code that calls the kernel, and mg_solver.c refers to it weakly
 * (mg_solver_internal.h): a build without it runs the 91-byte passes.
 */
#include "mg_solver_internal.h"
#include "mgk_sweep3.h"
#include <stddef.h>

/* the kernel is built for level 0's shape (whole 3-D grids with rows of 512 / 1024) */
int mg_triple_mid_fits(const mg_solver *s) {
    const mg_level *L = &s->L[0];
    return s->cfg.dim == 3 && !L->distributed && mgk_jacobi3_mid_ok_f64(&L->f[0].g);
}

/* tmp = J(J(J(u))) on level 0, *sumsq = || b - A J(u) ||^2.  Not timed with the two-sweep launches (profile kind 1 describes those) */
int mg_triple_mid_pass(mg_solver *s, double *sumsq) {
    mg_level *L = &s->L[0];
    mg_fset *F = &L->f[0];
    CHK(mgk_jacobi3_sumsq_mid_f64(s->ctx, &F->g, L->coef, L->dinv, s->cfg.scale, (const double *)F->b, (const double *)F->u, (double *)F->tmp,
                                  sumsq, NULL));
    return 0;
}
