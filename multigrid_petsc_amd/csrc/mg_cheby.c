/*
 * mg_cheby.c -- KSPCHEBYSHEV on the fused cycle (fuse bit 15, include/mgsolve.h).  PETSc's KSPSolve restarts the three-term recurrence at
 * every call, and the cycle calls it with max_it = v0: with v0 = 3 a smoothing is exactly the steps
 *
 *   p1 = p0 + s z(p0)                                   s = 2 / (emax + emin); from the zero guess p1 = s (b dinv)
 *   p2 = ((1 - w1) p0 + w1 p1) + (w1 Gamma s) z(p1)
 *   p3 = ((1 - w2) p1 + w2 p2) + (w2 Gamma s) z(p2)     z(p) = (b - A p) dinv
 *
 * of which only p3 is needed afterwards: one pass of the three-sweep 2-D kernel (mgk_cheby3_2d_*), whose extra operands p0 and p1 at the
 * point itself are still in its registers.  The levels that fit in LDS run in the tail kernel (mgk_tail_cycle_cheby_f64), 2-D and 3-D,
 * any step counts.  mg_solver.c decides WHERE these run (j3_2d_ok, the tail and graph conditions) and keeps the swap discipline; this
 * file is the only host code that calls the kernels, and mg_solver.c refers to it weakly (mg_solver_internal.h).
 */
#include "mg_solver_internal.h"
#include <stddef.h>

/* {s, (1 - w, w, w Gamma s) of step 2, of step 3}: the factors smooth_chebyshev passes to its step-by-step launches (mg_cheby_coefs.h) */
static void cheb7(const mg_solver *s, double *c) {
    mg_cheby_rec rec;
    mg_cheby_begin(&rec, s->cfg.emin, s->cfg.emax);
    c[0] = rec.scale;
    mg_cheby_next(&rec, c + 1);
    mg_cheby_next(&rec, c + 4);
}

int mg_cheby_pass(mg_solver *s, int l, int kind, double *sumsq) {
    mg_level *L = &s->L[l];
    mg_fset *F = &L->f[0];
    const int mesh = s->cfg.mesh != 0;                   /* -mesh 1/2: the row-table forms of the same kernels */
    const double *coef = mesh ? NULL : L->coef, *ctab = mesh ? L->ctab : NULL, *dtab = mesh ? L->dtab : NULL;
    const double dinv = mesh ? 1.0 : L->dinv;
    const double *b = (const double *)F->b, *u = (const double *)F->u;
    double *out = (double *)F->tmp;
    double c[7];
    cheb7(s, c);
    switch (kind) {
    case MG_CHEBY_ZERO:
        CHK(mgk_cheby3_2d_zero_f64(s->ctx, &F->g, coef, dinv, c, ctab, dtab, b, out, NULL));
        return 0;
    case MG_CHEBY_PLAIN:
        CHK(mgk_cheby3_2d_f64(s->ctx, &F->g, coef, dinv, c, ctab, dtab, b, u, out, NULL));
        return 0;
    case MG_CHEBY_PROLONG: {
        if (l + 1 >= s->levels) return mgi_fail(MGK_EINVAL, "mg_cheby_pass: no coarser level to prolong from");
        const mg_fset *C = &s->L[l + 1].f[0];
        CHK(mgk_prolong_cheby3_2d_f64(s->ctx, &F->g, &C->g, coef, dinv, c, ctab, dtab, b, (const double *)C->u, u, out, NULL));
        return 0;
    }
    case MG_CHEBY_NORM:
        if (!sumsq) return mgi_fail(MGK_EINVAL, "mg_cheby_pass: the norm pass needs a destination");
        CHK(mgk_cheby3_2d_sumsq_f64(s->ctx, &F->g, coef, dinv, c, ctab, dtab, b, u, out, sumsq, NULL));
        return 0;
    }
    return mgi_fail(MGK_EINVAL, "mg_cheby_pass: unknown kind");
}

/* b of level ltail in, its u after the post-smoothing out (mg_solver.c: tail()) */
int mg_cheby_tail(mg_solver *s) {
    const int lt = s->ltail, nl = s->levels - lt;
    int n[8];
    double k7[8 * 7], di[8];
    const double *ct[8], *dt[8];
    if (lt < 1 || nl < 1 || nl > 8) return mgi_fail(MGK_EINVAL, "mg_cheby_tail: no tail levels");
    for (int q = 0; q < nl; q++) {
        const mg_level *L = &s->L[lt + q];
        n[q] = L->n; di[q] = L->dinv;
        for (int e = 0; e < 7; e++) k7[7 * q + e] = L->coef[e];
        ct[q] = L->ctab; dt[q] = L->dtab;
    }
    mg_fset *F = &s->L[lt].f[0];
    const int mesh = s->cfg.mesh != 0;
    CHK(mgk_tail_cycle_cheby_f64(s->ctx, &F->g, nl, n, k7, di, mesh ? ct : NULL, mesh ? dt : NULL, s->cfg.emin, s->cfg.emax,
                                 s->cfg.v[0], s->cfg.v[1], (const double *)F->b, (double *)F->u, NULL));
    return 0;
}
