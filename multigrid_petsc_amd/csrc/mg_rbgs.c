/*
 * mg_rbgs.c -- red-black Gauss-Seidel smoothing (pc_type MG_PC_RBGS, include/mgsolve.h).  Point (i, j) of a level has the
 * colour (i + j) & 1; one sweep updates colour 0, then colour 1 from the new values, every point by
 *
 *   u <- u + scale ((b - A u) / diag)          (the expression of point Jacobi; scale is the relaxation factor, 1 is plain Gauss-Seidel)
 *
 * A smoothing of v sweeps is v / 2 passes of two sweeps and, if v is odd, one of one sweep (mgk_rbgs_2d_f64); from the zero guess the first
 * pass does not read u; with fuse bit 1 the first post-smoothing pass also prolongs and corrects (mgk_prolong_rbgs_2d_f64).  Every pass
 * reads u, writes tmp and swaps them -- the zero-guess pass like any other -- so pre- and post-smoothing of v0 sweeps swap (v0 + 1) / 2 times
 * each: an even count per level and cycle whatever v0, and the pointers a recorded coarse-level graph holds stay valid (the coarsest level,
 * with its one smoothing of v1 sweeps, is copied back by mg_solver.c after an odd count).  The uniform mesh runs on the level's constants, the
 * stretched meshes on the row tables.  This file is the only host code that calls the two kernels; mg_solver.c refers to it weakly
 * (mg_solver_internal.h).
 */
#include "mg_solver_internal.h"

static void rb_swap(mg_fset *F) {
    void *t = F->u; F->u = F->tmp; F->tmp = t;
    mgi_u_rewritten(F);
}

/* `sweeps` sweeps in passes of two and a last one of one; zero: the first pass starts from the zero guess */
static int rb_passes(mg_solver *s, int l, int sweeps, int zero) {
    mg_level *L = &s->L[l];
    mg_fset *F = &L->f[0];
    const double *ct = s->cfg.mesh ? L->ctab : NULL, *dt = s->cfg.mesh ? L->dtab : NULL;
    while (sweeps > 0) {
        const int ns = sweeps >= 2 ? 2 : 1;
        CHK(mgk_rbgs_2d_f64(s->ctx, &F->g, L->coef, L->dinv, s->cfg.scale, ct, dt, ns, (const double *)F->b, zero ? NULL : (const double *)F->u,
                            (double *)F->tmp, NULL));
        rb_swap(F);
        zero = 0;
        sweeps -= ns;
    }
    return 0;
}

/* KSPSolve(ksp[l], b[l], u[l]) with max_it = maxit */
int mg_rbgs_smooth(mg_solver *s, int l, int maxit) {
    mg_fset *F = &s->L[l].f[0];
    if (maxit <= 0) {
        if (!F->guess_nonzero) CHK(mgk_memset0(s->ctx, F->u, sizeof(double) * (size_t)F->g.total, NULL));   /* KSPSolve zero-fills */
        return 0;
    }
    return rb_passes(s, l, maxit, !F->guess_nonzero);
}

/* u_l <- RB^maxit(u_l + P u_{l+1}), maxit >= 1 */
int mg_rbgs_prolong_smooth(mg_solver *s, int l, int maxit) {
    mg_level *L = &s->L[l];
    mg_fset *F = &L->f[0], *Cq = &s->L[l + 1].f[0];
    const double *ct = s->cfg.mesh ? L->ctab : NULL, *dt = s->cfg.mesh ? L->dtab : NULL;
    const int ns = maxit >= 2 ? 2 : 1;
    if (maxit < 1) return mgi_fail(MGK_EINVAL, "mg_rbgs_prolong_smooth: needs at least one sweep");
    CHK(mgk_prolong_rbgs_2d_f64(s->ctx, &F->g, &Cq->g, L->coef, L->dinv, s->cfg.scale, ct, dt, ns, (const double *)F->b, (const double *)Cq->u,
                                (const double *)F->u, (double *)F->tmp, NULL));
    rb_swap(F);
    return rb_passes(s, l, maxit - ns, 0);
}
