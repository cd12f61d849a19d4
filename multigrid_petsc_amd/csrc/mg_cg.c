/*
 * mg_cg.c -- conjugate gradients with the V-cycle as preconditioner (PETSc's -ksp_type cg -pc_type mg) on the product's own driver:
 * mg_solver_solve_cg (include/mgsolve.h).  For the uniform mesh, where the fine-level operator A and the cycle operator
 * M = one V(v0,v0) cycle rooted at level 0 from the zero guess (mgi_apply_cycle: the fused passes, the coarse-level graph and the LDS tail of
 * the plain solve) are both symmetric:
 *
 *   x = 0, r = b, z = M r, p = z, rho = r . z
 *   step k:  q = A p;  sigma = p . q;  alpha = rho / sigma;  breakdown unless alpha is finite and > 0
 *            x = x + alpha p;  r = r - alpha q;  rnorm[k] = sqrt(r . r)
 *            stop: rnorm[k] <= rtol ||b||, k = maxiter, or the divergence guard of src/solver.c:1530
 *            z = M r;  rho' = r . z;  beta = rho' / rho;  breakdown unless beta is finite and >= 0;  p = z + beta p;  rho = rho'
 *
 * The level operator is NEGATIVE definite, so rho and sigma are both negative and alpha is positive: the signs of alpha and beta are tested,
 * never those of rho or sigma.  r is the recurrence residual with no preconditioner between it and b - A x: the stop rule of the plain solve
 * carries over unchanged.  r lives in level 0's b, where the cycle reads it; the caller's b is kept in a field of its own and copied back at the
 * end; z is level 0's u after the cycle.
 * Per step: one cycle, the 16 B dot r . z (mgk_multi_dot_f64 with k = 1), the 32 B direction pass (p = z + beta p, q = A p and sigma in one
 * pass; the two p buffers swap) and the 48 B update pass (x, r and r . r in one pass): 96 B per fine unknown beside the cycle and THREE host
 * synchronisations, for rho', sigma and r . r.  Five fine-level fields whatever the step count: x, p, the other p, q, the copy of b.
 *
 * This file is the only host code that calls the kernels of include/mgk_cg.h: mg_solver.c references nothing defined here and frees the fields
 * and the workspace through the solver's struct.
 */
#include "mg_solver_internal.h"
#include "mgk_cg.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int cg_check(const mg_solver *s) {
    if (!s) return mgi_fail(MGK_EINVAL, "mg_solver_solve_cg: null solver");
    if (s->cfg.nranks > 1) return mgi_fail(MGK_EINVAL, "mg_solver_solve_cg: built for one GPU (nranks == 1)");
    if (s->cfg.precision != MG_PREC_FP64) return mgi_fail(MGK_EINVAL, "mg_solver_solve_cg: built for fp64 (not mixed precision: use mg_solver_solve_cg_mixed)");
    if (s->cfg.ksp_type != MG_KSP_RICHARDSON) return mgi_fail(MGK_EINVAL, "mg_solver_solve_cg: built for Richardson + Jacobi (not Chebyshev)");
    if (s->cfg.pc_type != MG_PC_JACOBI)
        return mgi_fail(MGK_EINVAL, "mg_solver_solve_cg: built for point Jacobi (not the line or red-black Gauss-Seidel smoothers: their cycle is not symmetric)");
    if (s->cfg.mesh != 0)
        return mgi_fail(MGK_EINVAL, "mg_solver_solve_cg: built for the uniform mesh (mesh == 0): on a stretched mesh the operator and the cycle "
                                    "are not symmetric; use mg_solver_solve_gmres");
    return 0;
}

static void cg_ws_free(mgk_ctx *ctx, void *ws) { mgk_cg_workspace_destroy(ctx, (mgk_cg_ws *)ws); }

static void cg_free(mg_solver *s) {
    for (int q = 0; q < MG_CG_FIELDS; q++) if (s->cg_field[q]) mgk_free(s->ctx, s->cg_field[q]);
    memset(s->cg_field, 0, sizeof(s->cg_field));
    if (s->cg_rho_dev) mgk_free(s->ctx, s->cg_rho_dev);
    s->cg_rho_dev = NULL;
    if (s->cg_ws) cg_ws_free(s->ctx, s->cg_ws);
    s->cg_ws = NULL;
}

/* x, p, the other p, q and the copy of b, the device slot of r . z and the reduction workspace: allocated at the first call of either CG
 * driver (mg_cg_mixed.c shares them) */
int mgi_cg_alloc(mg_solver *s, const char *who) {
    if (s->cg_ws) return 0;
    CHK(mgk_sync(s->ctx, NULL));
    const size_t bytes = sizeof(double) * (size_t)s->L[0].f[0].g.total;
    s->cg_ws_free = cg_ws_free;
    for (int q = 0; q < MG_CG_FIELDS; q++) {
        if (mgk_malloc(s->ctx, &s->cg_field[q], bytes)) {
            char msg[256];
            snprintf(msg, sizeof(msg), "%s: needs %d fine-level fields of %zu bytes (%.3f GB in all): the device could not "
                     "allocate them", who, MG_CG_FIELDS, bytes, 1e-9 * (double)MG_CG_FIELDS * (double)bytes);
            cg_free(s);
            return mgi_fail(MGK_EINVAL, msg);
        }
    }
    void *q = NULL;
    mgk_cg_ws *ws = NULL;
    int rc = mgk_malloc(s->ctx, &q, sizeof(double));
    s->cg_rho_dev = (double *)q;
    if (!rc) rc = mgk_cg_workspace_create(s->ctx, &ws);
    if (rc) {
        char msg[128];
        snprintf(msg, sizeof(msg), "%s: the reduction workspace", who);
        cg_free(s);
        return mgi_fail(rc, msg);
    }
    s->cg_ws = ws;
    return 0;
}

static int cg_go_on(const mg_solver *s, double res, double tol) { return s->iter < s->cfg.maxiter && 100000000 * s->bnorm > res && res > tol; }

static int cg_run(mg_solver *s) {
    mg_level *L = &s->L[0];
    mg_fset *F = &L->f[0];
    const mgk_geom *g = &F->g;
    const size_t bytes = sizeof(double) * (size_t)g->total;
    double *x = (double *)s->cg_field[0], *p = (double *)s->cg_field[1], *pnew = (double *)s->cg_field[2], *q = (double *)s->cg_field[3];
    double *b0 = (double *)s->cg_field[4];
    double *r = (double *)F->b;                                       /* what the cycle reads (never swapped) */
    mgk_cg_ws *ws = (mgk_cg_ws *)s->cg_ws;
    const double tol = s->cfg.rtol * s->bnorm;
    double rho = 0.0, beta = 0.0, res = s->bnorm;
    CHK(mgk_d2d(s->ctx, b0, r, bytes, NULL));
    CHK(mgk_memset0(s->ctx, x, bytes, NULL));
    CHK(mgi_apply_cycle(s));                                           /* z = M r, in u */
    const double *rv[1] = {r};
    CHK(mgk_multi_dot_f64(s->ctx, g, 1, rv, (const double *)F->u, s->cg_rho_dev, &rho, NULL));
    for (int k = 1;; k++) {
        double sigma = 0.0, ss = 0.0;
        /* p = z + beta p into the other buffer (the first step: p = z, the old p is not read), q = A p, sigma = p . q */
        CHK(mgk_cg_direction_apply_dot_f64(s->ctx, g, L->coef, beta, (const double *)F->u, k == 1 ? NULL : p, pnew, q, ws, &sigma, NULL));
        { double *t = p; p = pnew; pnew = t; }
        const double alpha = rho / sigma;
        if (!(isfinite(alpha) && alpha > 0.0)) { s->cg_breakdown = k; break; }
        CHK(mgk_cg_update_sumsq_f64(s->ctx, g, alpha, p, q, x, r, ws, &ss, NULL));
        res = sqrt(ss);
        s->iter = k;
        s->rnorm[k] = res;
        if (!cg_go_on(s, res, tol)) break;
        CHK(mgi_apply_cycle(s));
        double rho1 = 0.0;
        CHK(mgk_multi_dot_f64(s->ctx, g, 1, rv, (const double *)F->u, s->cg_rho_dev, &rho1, NULL));
        beta = rho1 / rho;
        if (!(isfinite(beta) && beta >= 0.0)) { s->cg_breakdown = k; break; }
        rho = rho1;
    }
    CHK(mgk_d2d(s->ctx, F->u, x, bytes, NULL));
    CHK(mgk_d2d(s->ctx, r, b0, bytes, NULL));                          /* level 0's b is the caller's right-hand side again */
    F->guess_nonzero = 1;                                              /* u holds an iterate: mg_solver_cycles would continue from it */
    s->rchk = res;
    return 0;
}

int mg_solver_solve_cg(mg_solver *s) {
    int rc = cg_check(s);
    if (rc) return rc;
    rc = mgi_cg_alloc(s, "mg_solver_solve_cg");
    if (rc) return rc;
    mg_fset *F = &s->L[0].f[0];
    double ss = 0.0;
    CHK(mgk_sumsq_f64(s->ctx, &F->g, (const double *)F->b, &ss, NULL));
    s->bnorm = sqrt(ss);
    s->iter = 0;
    s->rnorm[0] = s->bnorm;
    s->rchk = s->bnorm;
    s->started = 1;
    s->cg_breakdown = 0;
    CHK(mgk_sync(s->ctx, NULL));
    const double t0 = mgi_wall();
    if (s->bnorm == 0.0 || s->cfg.maxiter < 1) CHK(mgk_memset0(s->ctx, F->u, sizeof(double) * (size_t)F->g.total, NULL));
    else CHK(cg_run(s));
    CHK(mgk_sync(s->ctx, NULL));
    s->solve_seconds = mgi_wall() - t0;
    return 0;
}

int mg_solver_cg_breakdown(const mg_solver *s) { return s ? s->cg_breakdown : 0; }
