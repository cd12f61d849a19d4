/*
 * mg_fmg.c -- full multigrid (nested iteration, PETSc's -pc_mg_type full) on the product's own driver: mg_solver_fmg and
 * mg_solver_solve_fmg (include/mgsolve.h).  Levels 0 (finest) .. L-1, operators, transfers and smoother of the V-cycle:
 *
 *   b_l = R b_{l-1}, l = 1 .. L-1                      full weighting (mgk_restrict_fw_f64)
 *   u_{L-1} = v1 sweeps on b_{L-1} from the zero guess  the V-cycle's coarsest treatment
 *   for l = L-2 .. 0:  u_l = 0 + P u_{l+1},  then nu V-cycles on the levels l .. L-1 from that guess (level l in the role of level 0)
 *
 * The result is u_0; FMG counts as iteration 1 (rnorm[1] = ||b_0 - A_0 u_0||) and the V-cycles that follow continue from it.
 * Hot path: the interpolation and the first pre-smoothing sweeps of the cycle that starts from it are ONE pass that never reads the old
 * iterate (mgk_interp_jacobi2_f64, 3-D; mgk_interp_jacobi3_2d_f64, 2-D), and every stage rooted on the levels that fit in LDS is one
 * launch (mgk_tail_fmg_f64).  Elsewhere, and where those kernels are not built for the shape or v0, a zeroed field and
 * mgk_prolong_add_f64 make the same bits.  The cycles themselves are mg_solver.c's (mg_solver_internal.h).
 *
 * This file is the only host code that calls the FMG kernels: mg_solver.c references nothing defined here.
 */
#include "mg_solver_internal.h"
#include <stdlib.h>
#include <string.h>

static int fmg_check(const mg_solver *s, int nu) {
    if (!s) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: null solver");
    if (nu < 1) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: nu must be >= 1");
    if (s->cfg.nranks > 1) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: built for one GPU (nranks == 1)");
    if (s->cfg.precision != MG_PREC_FP64) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: built for fp64 (not mixed precision)");
    if (s->cfg.ksp_type != MG_KSP_RICHARDSON) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: built for Richardson + Jacobi (not Chebyshev)");
    if (s->cfg.pc_type == MG_PC_LINE_Y) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: built for point Jacobi (not the y-line smoother)");
    if (s->cfg.pc_type == MG_PC_RBGS) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: built for point Jacobi (not the red-black Gauss-Seidel smoother)");
    if (s->cfg.pc_type != MG_PC_JACOBI) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: built for point Jacobi (not the x-line or alternating line smoothers)");
    if (s->cfg.mesh != 0) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: built for the uniform mesh (-mesh 0)");
    if (s->levels < 2) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: needs two levels or more");
    return 0;
}

/* u_l = 0 + P u_{l+1}; level l's KSP then starts from that guess.  With the interpolation kernel the pass also makes the first sweeps of
 * that smoothing (pre_done: smooth() starts after them) */
static int interpolate(mg_solver *s, int l) {
    mg_level *Lf = &s->L[l];
    mg_fset *F = &Lf->f[0], *C = &s->L[l + 1].f[0];
    const int v0 = s->cfg.v[0], fused = (s->cfg.fuse & MG_FUSE_PROLONG_SWEEP) != 0;
    F->guess_nonzero = 1;
    F->pre_done = 0; F->jz_ready = 0; F->last_sweep_pending = 0;
    if (fused && s->cfg.dim == 3 && v0 >= 2 && mgk_interp_jacobi2_ok_f64(&F->g, &C->g)) {
        CHK(mgk_interp_jacobi2_f64(s->ctx, &F->g, &C->g, Lf->coef, Lf->dinv, s->cfg.scale, (const double *)F->b, (const double *)C->u,
                                   (double *)F->u, NULL));
        F->pre_done = 2;
    } else if (fused && s->cfg.dim == 2 && v0 >= 3) {
        CHK(mgk_interp_jacobi3_2d_f64(s->ctx, &F->g, &C->g, Lf->coef, Lf->dinv, s->cfg.scale, (const double *)F->b, (const double *)C->u,
                                      (double *)F->u, NULL));
        F->pre_done = 3;
    } else {
        CHK(mgk_memset0(s->ctx, F->u, sizeof(double) * (size_t)F->g.total, NULL));
        CHK(mgk_prolong_add_f64(s->ctx, &F->g, &C->g, (const double *)C->u, (double *)F->u, NULL));
    }
    mgi_u_rewritten(F);
    return 0;
}

/* the stages rooted at the tail levels (ltail .. L-1) in one launch: b_ltail in, u_ltail after its own stage out */
static int tail_fmg(mg_solver *s, int nu) {
    const int lt = s->ltail, nl = s->levels - lt;
    int n[8];
    double k7[8 * 7], di[8];
    for (int q = 0; q < nl; q++) {
        const mg_level *L = &s->L[lt + q];
        n[q] = L->n; di[q] = L->dinv;
        for (int e = 0; e < 7; e++) k7[7 * q + e] = L->coef[e];
    }
    mg_fset *F = &s->L[lt].f[0];
    CHK(mgk_tail_fmg_f64(s->ctx, &F->g, nl, n, k7, di, s->cfg.scale, s->cfg.v[0], s->cfg.v[1], nu, (const double *)F->b, (double *)F->u, NULL));
    mgi_u_rewritten(F);
    return 0;
}

/* FMG(nu) from the state start() leaves */
static int fmg_run(mg_solver *s, int nu) {
    const int levels = s->levels, lt = s->ltail;
    if (s->rnorm_cap < 2) {
        double *r = (double *)realloc(s->rnorm, 2 * sizeof(double));
        if (!r) return mgi_fail(MGK_EINVAL, "mg_solver_fmg: out of host memory");
        s->rnorm = r; s->rnorm_cap = 2;
    }
    /* which buffer of each coarse level is u: the coarse-level graph of the V-cycles holds them as recorded, the stages below may swap */
    void *u_at[MG_MAX_LEVELS];
    for (int l = 1; l < levels; l++) u_at[l] = s->L[l].f[0].u;
    const int lchain = lt ? lt : levels - 1;
    for (int l = 1; l <= lchain; l++) {                                  /* b_l = R b_{l-1} */
        mg_fset *F = &s->L[l - 1].f[0], *C = &s->L[l].f[0];
        CHK(mgk_restrict_fw_f64(s->ctx, &F->g, &C->g, (const double *)F->b, (double *)C->b, NULL));
    }
    int top;                                                            /* the finest level solved so far */
    if (lt) {
        CHK(tail_fmg(s, nu));
        top = lt;
    } else {
        mg_fset *Z = &s->L[levels - 1].f[0];
        Z->guess_nonzero = 0; Z->jz_ready = 0;
        CHK(mgi_smooth(s, levels - 1, s->cfg.v[1]));
        top = levels - 1;
    }
    for (int l = top - 1; l >= 1; l--) {
        CHK(interpolate(s, l));
        for (int q = 0; q < nu; q++) CHK(mgi_vcycle_rooted(s, l));
        s->L[l].f[0].guess_nonzero = 0;                                 /* an inner level of every cycle from here on */
    }
    CHK(interpolate(s, 0));
    for (int l = 1; l < levels; l++) {                                  /* their contents are spent: back to the recorded buffer roles */
        mg_fset *F = &s->L[l].f[0];
        /* needed for the RESULT, not for speed alone: the re-record check of cycle_body watches the level that feeds the recording, not the
         * levels inside it.  A stage level can swap u / tmp an odd number of times (the root's first pre-smoothing is shortened by pre_done,
         * the post-smoothing is not); a recording made by an earlier cycle then leaves level lgraph's result in the buffer that was u when it
         * was recorded, while the prolongation to the level above reads the one that is u now.  Seen with the tail off, the graph on and a
         * second FMG on a live handle (tools/stress_sessions_mock.py; the fixed sessions of tests/san_fmg.c) */
        if (F->u != u_at[l]) { void *t = F->u; F->u = F->tmp; F->tmp = t; }
        /* a guard, not a repair: every flag is 0 already.  guess_nonzero: the stage loop above for the stage roots, mgi_vcycle_rooted for the levels
         * below a root, mgi_start for the tail levels and the coarsest one.  jz_ready is set by a restriction and consumed by the smoothing
         * (or the tail kernel) that follows it in the same descent; last_sweep_pending is set by a pre-smoothing and consumed by the
         * restriction that follows it; pre_done is set by interpolate() and consumed by the first smoothing of the nu >= 1 cycles of that
         * stage.  No session can tell this line from its absence while every stage ends on a complete cycle; it stays so that a stage
         * that does not (nu = 0, an early exit) cannot leak a flag into the solver's own cycles, where a stale jz_ready skips a sweep */
        F->guess_nonzero = 0; F->jz_ready = 0; F->last_sweep_pending = 0; F->pre_done = 0;
    }
    s->last_cycle = 0;
    for (int q = 0; q < nu; q++) CHK(mgi_vcycle_once(s));              /* the stage rooted at level 0: the solver's own cycle + norm */
    s->iter = 1;                                                        /* FMG is iteration 1 */
    s->rnorm[1] = s->rchk;
    return 0;
}

int mg_solver_fmg(mg_solver *s, int nu) {
    int rc = fmg_check(s, nu);
    if (rc) return rc;
    CHK(mgi_start(s));
    return fmg_run(s, nu);
}

int mg_solver_solve_fmg(mg_solver *s, int nu) {
    int rc = fmg_check(s, nu);
    if (rc) return rc;
    CHK(mgi_start(s));
    CHK(mgk_sync(s->ctx, NULL));
    const double t0 = mgi_wall();
    CHK(fmg_run(s, nu));
    CHK(mgi_iterate(s));                                                /* V-cycles under the stop rule of src/solver.c:1530 */
    CHK(mgi_finalize(s));
    CHK(mgk_sync(s->ctx, NULL));
    s->solve_seconds = mgi_wall() - t0;
    return 0;
}
