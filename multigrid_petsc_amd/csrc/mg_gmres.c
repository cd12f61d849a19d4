/*
 * mg_gmres.c -- restarted GMRES with the V-cycle as RIGHT preconditioner (PETSc's -ksp_type gmres -pc_type mg -ksp_pc_side right) on the
 * product's own driver: mg_solver_solve_gmres (include/mgsolve.h).  M = one cycle rooted at level 0 from the zero guess (mgi_apply_cycle:
 * the fused passes, the coarse-level graph and the LDS tail of the plain solve), A = the fine-level operator.  Classical Gram-Schmidt in one
 * pass without refinement, PETSc's defaults:
 *
 *   x = 0, r = b, beta = ||b||, v_0 = r / beta, g = beta e_0
 *   step j:  z = M v_j;  w = A z;  h_i = v_i . w (i <= j), one pass;  w -= sum h_i v_i and h_{j+1} = ||w||, one pass;
 *            Givens rotations on the host: |g_{j+1}| is ||b - A x_j|| of the iterate this basis would give;  v_{j+1} = w / h_{j+1}
 *   stop (|g_{j+1}| <= rtol ||b||, maxiter steps, the divergence guard of src/solver.c:1530) or `restart` steps made:
 *            H y = g (triangular), t = V y, x += M t;  going on: r = b - A x, beta = ||r||, v_0 = r / beta
 *
 * With right preconditioning the estimate is the norm of the TRUE residual, so the stop rule of the plain solve carries over unchanged.
 * One host synchronisation per step: the read of h and ||w||^2 (mgk_krylov_fetch); the two orthogonalisation passes run back to back, the
 * second one reading h from device memory.  v_j reaches the cycle by being written to level 0's b as well (mgk_scale_to_f64's second
 * destination: 8 B per unknown, no copy); the caller's b is kept in a field of its own and copied back at the end.
 *
 * This file is the only host code that calls the mgk_multi_dot_f64 / mgk_multi_axpy_sumsq_f64 / mgk_krylov_fetch / mgk_lincomb_f64 /
 * mgk_scale_to_f64 kernels: mg_solver.c references nothing defined here.
 */
#include "mg_solver_internal.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define KM MGK_KRYLOV_MAX

static int gmres_check(const mg_solver *s, int restart) {
    if (!s) return mgi_fail(MGK_EINVAL, "mg_solver_solve_gmres: null solver");
    if (restart < 1 || restart > KM - 1) return mgi_fail(MGK_EINVAL, "mg_solver_solve_gmres: restart must be within 1 .. MGK_KRYLOV_MAX - 1 (32)");
    if (s->cfg.nranks > 1) return mgi_fail(MGK_EINVAL, "mg_solver_solve_gmres: built for one GPU (nranks == 1)");
    if (s->cfg.precision != MG_PREC_FP64) return mgi_fail(MGK_EINVAL, "mg_solver_solve_gmres: built for fp64 (not mixed precision)");
    if (s->cfg.ksp_type != MG_KSP_RICHARDSON) return mgi_fail(MGK_EINVAL, "mg_solver_solve_gmres: built for Richardson + Jacobi (not Chebyshev)");
    if (s->cfg.pc_type == MG_PC_LINE_Y) return mgi_fail(MGK_EINVAL, "mg_solver_solve_gmres: built for point Jacobi (not the y-line smoother)");
    if (s->cfg.pc_type == MG_PC_RBGS) return mgi_fail(MGK_EINVAL, "mg_solver_solve_gmres: built for point Jacobi (not the red-black Gauss-Seidel smoother)");
    if (s->cfg.pc_type != MG_PC_JACOBI) return mgi_fail(MGK_EINVAL, "mg_solver_solve_gmres: built for point Jacobi (not the x-line or alternating line smoothers)");
    return 0;
}

static void gmres_free(mg_solver *s) {
    for (int q = 0; q < s->gm_nfields; q++) if (s->gm_field[q]) mgk_free(s->ctx, s->gm_field[q]);
    memset(s->gm_field, 0, sizeof(s->gm_field));
    s->gm_nfields = 0; s->gm_restart = 0;
}

/* basis (restart + 1 fields), x, w and the copy of b: allocated at the first call for this restart length */
static int gmres_alloc(mg_solver *s, int restart) {
    if (s->gm_restart == restart && s->gm_nfields == restart + 4) return 0;
    CHK(mgk_sync(s->ctx, NULL));
    gmres_free(s);
    const size_t bytes = sizeof(double) * (size_t)s->L[0].f[0].g.total;
    const int nf = restart + 4;
    if (!s->gm_hdev) {
        void *q = NULL;
        CHK(mgk_malloc(s->ctx, &q, sizeof(double) * (KM + 1)));
        s->gm_hdev = (double *)q;
    }
    s->gm_nfields = nf;
    for (int q = 0; q < nf; q++) {
        if (mgk_malloc(s->ctx, &s->gm_field[q], bytes)) {
            char msg[256];
            snprintf(msg, sizeof(msg), "mg_solver_solve_gmres: restart %d needs %d fine-level fields of %zu bytes (%.3f GB in all): the device "
                     "could not allocate them; choose a shorter restart", restart, nf, bytes, 1e-9 * (double)nf * (double)bytes);
            gmres_free(s);
            return mgi_fail(MGK_EINVAL, msg);
        }
    }
    s->gm_restart = restart;
    return 0;
}

/* y = A x on the fine level, in the canonical order */
static int apply_A(mg_solver *s, const double *x, double *y) {
    mg_level *L = &s->L[0];
    if (s->cfg.mesh) return mgk_rowcoef_f64(s->ctx, &L->f[0].g, 4, L->ctab, L->dtab, 1.0, NULL, x, y, NULL);
    return mgk_apply_f64(s->ctx, &L->f[0].g, L->coef, x, y, NULL);
}

static int gmres_run(mg_solver *s, int m) {
    mg_level *L = &s->L[0];
    mg_fset *F = &L->f[0];
    const mgk_geom *g = &F->g;
    const size_t bytes = sizeof(double) * (size_t)g->total;
    double **V = (double **)s->gm_field;                              /* V[0 .. m] */
    double *x = (double *)s->gm_field[m + 1], *w = (double *)s->gm_field[m + 2], *b0 = (double *)s->gm_field[m + 3];
    double *b = (double *)F->b;                                       /* what the cycle reads (never swapped) */
    double H[KM][KM], cs[KM], sn[KM], gv[KM + 1], y[KM], h[KM];       /* H[j] = column j after the rotations */
    const double tol = s->cfg.rtol * s->bnorm;
    double beta = s->bnorm, res = s->bnorm;
    int first = 1;                                                    /* x is still zero */
    CHK(mgk_d2d(s->ctx, b0, b, bytes, NULL));
    while (s->iter < s->cfg.maxiter && 100000000 * s->bnorm > res && res > tol) {
        /* v_0 = r / beta, into the basis and into the cycle's b */
        CHK(mgk_scale_to_f64(s->ctx, g, 1.0 / beta, first ? b0 : w, V[0], b, NULL));
        memset(gv, 0, sizeof(gv));
        gv[0] = beta;
        int j = 0, go = 1;
        while (go) {
            CHK(mgi_apply_cycle(s));                                                     /* z = M v_j, in u */
            CHK(apply_A(s, (const double *)F->u, w));                                   /* w = A z */
            CHK(mgk_multi_dot_f64(s->ctx, g, j + 1, (const double *const *)V, w, s->gm_hdev, NULL, NULL));
            CHK(mgk_multi_axpy_sumsq_f64(s->ctx, g, j + 1, s->gm_hdev, (const double *const *)V, w, NULL, NULL));
            double ss = 0.0;
            CHK(mgk_krylov_fetch(s->ctx, j + 1, h, &ss, NULL));                         /* the step's one synchronisation */
            const double hn = sqrt(ss);
            for (int i = 0; i < j; i++) {                                               /* the earlier rotations on the new column */
                const double t = cs[i] * h[i] + sn[i] * h[i + 1];
                h[i + 1] = cs[i] * h[i + 1] - sn[i] * h[i];
                h[i] = t;
            }
            const double d = sqrt(h[j] * h[j] + hn * hn);
            if (d == 0.0) { cs[j] = 1.0; sn[j] = 0.0; } else { cs[j] = h[j] / d; sn[j] = hn / d; }
            h[j] = cs[j] * h[j] + sn[j] * hn;
            gv[j + 1] = -(sn[j] * gv[j]);
            gv[j] = cs[j] * gv[j];
            for (int i = 0; i <= j; i++) H[j][i] = h[i];
            res = fabs(gv[j + 1]);
            s->iter++;
            s->rnorm[s->iter] = res;
            j++;
            go = j < m && s->iter < s->cfg.maxiter && 100000000 * s->bnorm > res && res > tol;   /* hn == 0 (breakdown) gives res == 0 */
            if (go) CHK(mgk_scale_to_f64(s->ctx, g, 1.0 / hn, w, V[j], b, NULL));
        }
        /* H y = g, t = V y into the cycle's b, x += M t */
        for (int i = j - 1; i >= 0; i--) {
            double t = gv[i];
            for (int q = i + 1; q < j; q++) t -= H[q][i] * y[q];
            y[i] = H[i][i] != 0.0 ? t / H[i][i] : 0.0;
        }
        CHK(mgk_lincomb_f64(s->ctx, g, j, y, (const double *const *)V, b, NULL));
        CHK(mgi_apply_cycle(s));
        const int more = s->iter < s->cfg.maxiter && 100000000 * s->bnorm > res && res > tol;
        if (first && !more) break;                                    /* u = M t is the solution: x was zero */
        if (first) CHK(mgk_d2d(s->ctx, x, F->u, bytes, NULL));
        else CHK(mgk_flat_axpy(s->ctx, g->total, 1.0, (const double *)F->u, x, NULL));
        first = 0;
        if (!more) { CHK(mgk_d2d(s->ctx, F->u, x, bytes, NULL)); break; }
        /* r = b - A x, beta = ||r|| : the next cycle of steps starts from the true residual */
        if (s->cfg.mesh) CHK(mgk_rowcoef_f64(s->ctx, g, 1, L->ctab, L->dtab, 1.0, b0, x, w, NULL));
        else CHK(mgk_residual_f64(s->ctx, g, L->coef, b0, x, w, NULL));
        double ss = 0.0;
        CHK(mgk_sumsq_f64(s->ctx, g, w, &ss, NULL));
        beta = sqrt(ss);
        res = beta;
        if (!(100000000 * s->bnorm > res && res > tol)) { CHK(mgk_d2d(s->ctx, F->u, x, bytes, NULL)); break; }
    }
    CHK(mgk_d2d(s->ctx, b, b0, bytes, NULL));                          /* level 0's b is the caller's right-hand side again */
    F->guess_nonzero = 1;                                              /* u holds an iterate: mg_solver_cycles would continue from it */
    s->rchk = res;
    return 0;
}

int mg_solver_solve_gmres(mg_solver *s, int restart) {
    int rc = gmres_check(s, restart);
    if (rc) return rc;
    rc = gmres_alloc(s, restart);
    if (rc) return rc;
    mg_fset *F = &s->L[0].f[0];
    double ss = 0.0;
    CHK(mgk_sumsq_f64(s->ctx, &F->g, (const double *)F->b, &ss, NULL));
    s->bnorm = sqrt(ss);
    s->iter = 0;
    s->rnorm[0] = s->bnorm;
    s->rchk = s->bnorm;
    s->started = 1;
    CHK(mgk_sync(s->ctx, NULL));
    const double t0 = mgi_wall();
    if (s->bnorm == 0.0 || s->cfg.maxiter < 1) CHK(mgk_memset0(s->ctx, F->u, sizeof(double) * (size_t)F->g.total, NULL));
    else CHK(gmres_run(s, restart));
    CHK(mgk_sync(s->ctx, NULL));
    s->solve_seconds = mgi_wall() - t0;
    return 0;
}
