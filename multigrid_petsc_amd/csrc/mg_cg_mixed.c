/*
 * mg_cg_mixed.c -- conjugate gradients in fp64 with the fp32 V-cycle of a mixed-precision solver as preconditioner: mg_solver_solve_cg_mixed
 * (include/mgsolve.h).  The recurrence of mg_cg.c (section 8l) with M r = (double) Vcycle32((float) r) from the zero
 * guess, the cycle the mixed iteration runs between its fp64 defect corrections.  F = level 0's fp64 set, E = its fp32 set:
 *
 *   x = 0, r = b (fp64, in F->b), r32 = (float) r (in E->b)
 *   z32 = Vcycle32(r32) (in E->u);  rho = sum r * (double) z32
 *   step k:  p = (double) z32 + beta p;  q = A p;  sigma = p . q;  alpha = rho / sigma;  breakdown unless alpha is finite and > 0
 *            x = x + alpha p;  r = r - alpha q;  rnorm[k] = sqrt(sum r^2);  r32 = (float) r
 *            stop: rnorm[k] <= rtol ||b||, k = maxiter, or the divergence guard of src/solver.c:1530
 *            z32 = Vcycle32(r32);  rho' = sum r * (double) z32;  beta = rho' / rho;  breakdown unless beta is finite and >= 0;  rho = rho'
 *
 * Every fp64 product and sum is rounded separately; (float) rounds to nearest, (double) is exact.  The fp32 cycle is symmetric to about 3e-7
 * only (|a . M b - b . M a| / |a . M b|); at rtol 1e-7 that costs no step against fp64 CG on the cases of tests/cg_mixed_reference.py.
 * Per step: one fp32 cycle, the 12 B dot, the 28 B direction pass (z read in fp32) and the 52-56 B update pass, which also stores r32 and, under
 * the condition of the mixed iteration (mgi_mixed_jz), the cycle's first zero-guess sweep e0 into E->tmp: 92-96 B per fine unknown beside the
 * cycle, three launches, three host synchronisations.  The fields and the workspace are those of mg_cg.c (mgi_cg_alloc).
 *
 * This file is the only host code that calls the kernels of include/mgk_cg_mixed.h.
 */
#include "mg_solver_internal.h"
#include "mgk_cg_mixed.h"
#include <math.h>
#include <string.h>

#define WHO "mg_solver_solve_cg_mixed"

static int cgm_check(const mg_solver *s) {
    if (!s) return mgi_fail(MGK_EINVAL, WHO ": null solver");
    if (s->cfg.precision != MG_PREC_MIXED)
        return mgi_fail(MGK_EINVAL, WHO ": built for a mixed-precision solver (precision = MG_PREC_MIXED; in fp64 use mg_solver_solve_cg)");
    if (s->cfg.nranks > 1) return mgi_fail(MGK_EINVAL, WHO ": built for one GPU (nranks == 1)");
    if (s->cfg.ksp_type != MG_KSP_RICHARDSON) return mgi_fail(MGK_EINVAL, WHO ": built for Richardson + Jacobi (not Chebyshev)");
    if (s->cfg.pc_type != MG_PC_JACOBI)
        return mgi_fail(MGK_EINVAL, WHO ": built for point Jacobi (not the line or red-black Gauss-Seidel smoothers: their cycle is not symmetric)");
    if (s->cfg.mesh != 0) return mgi_fail(MGK_EINVAL, WHO ": built for the uniform mesh (mesh == 0)");
    if (s->cfg.dim != 3) return mgi_fail(MGK_EINVAL, WHO ": built for 3-D (the fp32 cycle is)");
    return 0;
}

static int cgm_go_on(const mg_solver *s, double res, double tol) { return s->iter < s->cfg.maxiter && 100000000 * s->bnorm > res && res > tol; }

static int cgm_run(mg_solver *s) {
    mg_level *L = &s->L[0];
    mg_fset *F = &L->f[0], *E = &L->f[1];
    const mgk_geom *g = &F->g, *g32 = &E->g;
    const size_t bytes = sizeof(double) * (size_t)g->total;
    double *x = (double *)s->cg_field[0], *p = (double *)s->cg_field[1], *pnew = (double *)s->cg_field[2], *q = (double *)s->cg_field[3];
    double *b0 = (double *)s->cg_field[4];
    double *r = (double *)F->b;
    mgk_cg_ws *ws = (mgk_cg_ws *)s->cg_ws;
    const double tol = s->cfg.rtol * s->bnorm;
    const int jz = mgi_mixed_jz(s);                                    /* the update pass also makes the cycle's first sweep */
    double rho = 0.0, beta = 0.0, res = s->bnorm, ss = 0.0;
    CHK(mgk_d2d(s->ctx, b0, r, bytes, NULL));
    CHK(mgk_memset0(s->ctx, x, bytes, NULL));
    /* r32 = (float)(b - A 0) = (float) b bit for bit (and e0): the bridge pass of the mixed iteration on the zeroed x */
    if (jz) CHK(mgk_residual_f64_to_f32_jz(s->ctx, g, g32, L->coef, r, x, (float *)E->b, (float *)E->tmp, L->dinv, s->cfg.scale, &ss, NULL));
    else CHK(mgk_residual_f64_to_f32(s->ctx, g, g32, L->coef, r, x, (float *)E->b, &ss, NULL));
    CHK(mgi_apply_cycle_f32(s, jz));                                   /* z32 = Vcycle32(r32), in E->u */
    CHK(mgk_cg_dot_f64_f32(s->ctx, g, g32, r, (const float *)E->u, ws, &rho, NULL));
    for (int k = 1;; k++) {
        double sigma = 0.0;
        CHK(mgk_cg_direction_apply_dot_zf32_f64(s->ctx, g, g32, L->coef, beta, (const float *)E->u, k == 1 ? NULL : p, pnew, q, ws, &sigma, NULL));
        { double *t = p; p = pnew; pnew = t; }
        const double alpha = rho / sigma;
        if (!(isfinite(alpha) && alpha > 0.0)) { s->cg_breakdown = k; break; }
        CHK(mgk_cg_update_sumsq_f64_f32(s->ctx, g, g32, alpha, p, q, x, r, (float *)E->b, jz ? (float *)E->tmp : NULL, L->dinv, s->cfg.scale, ws, &ss, NULL));
        res = sqrt(ss);
        s->iter = k;
        s->rnorm[k] = res;
        if (!cgm_go_on(s, res, tol)) break;
        CHK(mgi_apply_cycle_f32(s, jz));
        double rho1 = 0.0;
        CHK(mgk_cg_dot_f64_f32(s->ctx, g, g32, r, (const float *)E->u, ws, &rho1, NULL));
        beta = rho1 / rho;
        if (!(isfinite(beta) && beta >= 0.0)) { s->cg_breakdown = k; break; }
        rho = rho1;
    }
    CHK(mgk_d2d(s->ctx, F->u, x, bytes, NULL));
    CHK(mgk_d2d(s->ctx, r, b0, bytes, NULL));                          /* level 0's b is the caller's right-hand side again */
    F->guess_nonzero = 1;
    mgi_u_rewritten(F);
    s->rchk = res;
    return 0;
}

int mg_solver_solve_cg_mixed(mg_solver *s) {
    int rc = cgm_check(s);
    if (rc) return rc;
    rc = mgi_cg_alloc(s, WHO);
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
    else CHK(cgm_run(s));
    CHK(mgk_sync(s->ctx, NULL));
    s->solve_seconds = mgi_wall() - t0;
    return 0;
}
