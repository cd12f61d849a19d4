/*
 * mg_line.c -- y-line Jacobi smoothing (pc_type MG_PC_LINE_Y, include/mgsolve.h).  One sweep of KSPRICHARDSON with
 * the y-tridiagonal part T of the level operator as preconditioner,
 *
 *   u <- u + scale T^-1 (b - A u),
 *
 * solved exactly in every column by the Thomas algorithm.  The operator rows depend on the grid row only, so T is the same matrix in every
 * column and its factorisation is three tables of n doubles per level, computed here once (C99 double, no FMA: -ffp-contract=off):
 *
 *   m_0 = C_0, g_0 = 1/m_0, l_0 = 0;   i >= 1: l_i = S_i g_{i-1}, m_i = C_i - l_i N_{i-1}, g_i = 1/m_i;   q_i = N_i g_i
 *
 * (band_factor, mg_line_factor.h, on the bands S, C, N of the row table).
 *
 * A sweep is a forward pass (residual, forward substitution, z = y g -> the level's tmp) and a backward pass (back substitution and the
 * update, in place in u): no buffer is swapped, so the pointers a recorded coarse-level graph holds stay valid whatever the sweep counts.
 * This file is the only host code that calls the two kernels; mg_solver.c refers to it weakly (mg_solver_internal.h).
 */
#include "mg_solver_internal.h"
#include "mg_line_factor.h"
#include <stdlib.h>

int mg_line_tables(mg_solver *s, int l, const double *ctab_host) {
    mg_level *L = &s->L[l];
    const size_t n = (size_t)L->n;
    double *h = (double *)malloc(sizeof(double) * 3 * n);
    if (!h) return mgi_fail(MGK_EINVAL, "mg_line_tables: out of host memory");
    band_factor(L->n, 5, ctab_host, ctab_host + 2, ctab_host + 4, h, h + n, h + 2 * n);
    int rc = mgi_upload(s, h, n, &L->ltab);
    if (!rc) rc = mgi_upload(s, h + n, n, &L->gtab);
    if (!rc) rc = mgi_upload(s, h + 2 * n, n, &L->qtab);
    free(h);
    return rc;
}

/* KSPSolve(ksp[l], b[l], u[l]) with max_it = maxit: from the zero guess the first sweep reads neither u nor the operator */
int mg_line_smooth(mg_solver *s, int l, int maxit) {
    mg_level *L = &s->L[l];
    mg_fset *F = &L->f[0];
    if (L->chunktab) return mg_line_chunk_smooth(s, l, maxit);    /* mg_config.line_chunk, a level with separators: mg_line_chunk.c's four passes */
    const double *b = (const double *)F->b;
    double *u = (double *)F->u, *z = (double *)F->tmp;
    if (maxit == 0 && !F->guess_nonzero) CHK(mgk_memset0(s->ctx, u, sizeof(double) * (size_t)F->g.total, NULL));   /* KSPSolve zero-fills */
    for (int it = 0; it < maxit; it++) {
        const double *uin = (it == 0 && !F->guess_nonzero) ? NULL : u;
        CHK(mgk_line_forward_f64(s->ctx, &F->g, L->ctab, L->ltab, L->gtab, b, uin, z, NULL));
        CHK(mgk_line_backward_f64(s->ctx, &F->g, L->qtab, s->cfg.scale, z, uin, u, NULL));
    }
    return 0;
}
