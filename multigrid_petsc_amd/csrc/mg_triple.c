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
 * (mg_solver_internal.h): a build without it runs the 91-byte passes.  Below it, the same bit's prolongation + three-sweep pass.
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

/* fuse bit 17 (MG_FUSE_TRIPLE_NORM): tmp = J(J(J(u))) on level 0, *sumsq = || b - A u ||^2 of u itself -- the complete
 * iterate the prolongation + three-sweep pass below left there -- so that the next cycle's pre-smoothing is this one pass:
 *
 *   (P + S1, S2, S3)  (N + S1', S2', S3')  (R)  =  25 + 24 + 17  =  66 B per fine unknown and cycle
 *
 * The stacked kernel with the norm of its input, four rows per wave (mgk_jacobi3_sumsq_f64 takes it on the shapes mg_triple_mid_fits accepts).
 * u is not modified: a solve that stops here owes no sweep.  mg_solver.c times the launch (profile kind 2); counted here */
int mg_triple_norm_pass(mg_solver *s, double *sumsq) {
    mg_level *L = &s->L[0];
    mg_fset *F = &L->f[0];
    CHK(mgk_jacobi3_sumsq_f64(s->ctx, &F->g, L->coef, L->dinv, s->cfg.scale, (const double *)F->b, (const double *)F->u, (double *)F->tmp, sumsq, NULL));
    s->triple_norm_launches++;
    return 0;
}

/* The prolongation form of the same kernel: where the post-smoothing of a level runs through the generic branch of
 * prolong_smooth() -- level 1 of a 1025^3 solve in every cycle, level 0 in the last cycle of a call -- (P + S1)(S2, S3) = 25 + 24 B becomes
 * (P + S1, S2, S3) = 25 B per unknown of that level.  The level swaps u / tmp once instead of twice: mg_solver.c takes the pass only on
 * levels whose pointers no recording holds. */
int mg_triple_prolong_fits(const mg_solver *s, int l) {
    if (s->cfg.dim != 3 || l < 0 || l + 1 >= s->levels) return 0;
    const mg_level *Lf = &s->L[l], *Lc = &s->L[l + 1];
    return !Lf->distributed && !Lc->distributed && mgk_prolong_jacobi3_ok_f64(&Lf->f[0].g, &Lc->f[0].g);
}

/* tmp = J(J(J(u + P u_{l+1}))) on level l.  Not timed as a profile kind (kinds 0 - 2 describe other launches); counted per level instead */
int mg_triple_prolong_pass(mg_solver *s, int l) {
    mg_level *L = &s->L[l];
    mg_fset *F = &L->f[0], *Cq = &s->L[l + 1].f[0];
    CHK(mgk_prolong_jacobi3_f64(s->ctx, &F->g, &Cq->g, L->coef, L->dinv, s->cfg.scale, (const double *)F->b, (const double *)Cq->u,
                                (const double *)F->u, (double *)F->tmp, NULL));
    s->prolong_triple_launches[l]++;
    return 0;
}
