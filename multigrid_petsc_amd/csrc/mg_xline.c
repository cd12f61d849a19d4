/*
 * mg_xline.c -- x-line Jacobi and alternating line smoothing (pc_type MG_PC_LINE_X / MG_PC_LINE_ALT, include/mgsolve.h; DESIGN.md section
 * 8g).  One x sweep of KSPRICHARDSON with the x-tridiagonal part T_x of the level operator as preconditioner,
 *
 *   u <- u + scale T_x^-1 (b - A u),
 *
 * solved exactly in every row by the Thomas algorithm.  In grid row i T_x is the constant-band matrix (W_i, C_i, E_i); its factorisation
 * along the columns is ONE table per level, computed here once (C99 double, no FMA: -ffp-contract=off):
 *
 *   m_{i,0} = C_i, g_{i,0} = 1/m_{i,0};   j >= 1: l_{i,j} = W_i g_{i,j-1}, t = l_{i,j} E_i, m_{i,j} = C_i - t, g_{i,j} = 1/m_{i,j}
 *
 * (the multipliers l_{i,j} and q_{i,j} = E_i g_{i,j} are one rounded product each, formed by the kernels).  On the uniform mesh every row
 * is the same: one row of n doubles, row stride 0.  On a stretched mesh n rows at a stride of n rounded up to 16 doubles (whole 128-byte
 * lines per row), the padding zero.
 * A sweep is a forward pass (residual, forward substitution, z = y g -> the level's tmp) and a backward pass (back substitution and the
 * update, in place in u): no buffer is swapped.  MG_PC_LINE_ALT: within one KSPSolve sweep k is a y-line sweep (mg_line.c) for even k and
 * an x-line sweep for odd k.  This file is the only host code that calls the two kernels; mg_solver.c refers to it weakly
 * (mg_solver_internal.h).  With mg_config.xline_chunk the x sweeps of a level that has separators are mg_xline_chunk.c's.
 */
#include "mg_solver_internal.h"
#include "mg_line_factor.h"
#include <stdlib.h>
#include <string.h>

long mg_xline_stride(int n, int uniform) { return uniform ? 0 : (long)round16((size_t)n); }

/* g of `rows` grid rows (1 on the uniform mesh: ctab's first row), n columns each, at a stride of gs doubles (0 allowed when rows == 1) */
void mg_xline_factor(int n, int rows, const double *ctab, long gs, double *g) {
    for (int i = 0; i < rows; i++) {
        const double *r = ctab + 5 * (size_t)i;
        double *gi = g + (size_t)i * (size_t)gs;
        double m = r[2];
        gi[0] = 1.0 / m;
        for (int j = 1; j < n; j++) {
            const double l = r[1] * gi[j - 1];
            const double t = l * r[3];
            m = r[2] - t;
            gi[j] = 1.0 / m;
        }
    }
}

int mg_xline_tables(mg_solver *s, int l, const double *ctab_host) {
    mg_level *L = &s->L[l];
    const int uniform = (s->cfg.mesh == 0), rows = uniform ? 1 : L->n;
    const long gs = mg_xline_stride(L->n, uniform);
    const size_t len = uniform ? (size_t)L->n : (size_t)rows * (size_t)gs;
    double *h = (double *)calloc(len, sizeof(double));
    if (!h) return mgi_fail(MGK_EINVAL, "mg_xline_tables: out of host memory");
    mg_xline_factor(L->n, rows, ctab_host, gs, h);
    const int rc = mgi_upload(s, h, len, &L->xgtab);
    L->xgs = gs;
    free(h);
    return rc;
}

/* KSPSolve(ksp[l], b[l], u[l]) with max_it = maxit: from the zero guess the first sweep reads neither u nor the operator */
int mg_xline_smooth(mg_solver *s, int l, int maxit) {
    mg_level *L = &s->L[l];
    mg_fset *F = &L->f[0];
    const double *b = (const double *)F->b;
    double *u = (double *)F->u, *z = (double *)F->tmp;
    const int guess = F->guess_nonzero, alt = (s->cfg.pc_type == MG_PC_LINE_ALT);
    if (maxit == 0 && !guess) CHK(mgk_memset0(s->ctx, u, sizeof(double) * (size_t)F->g.total, NULL));   /* KSPSolve zero-fills */
    for (int it = 0; it < maxit; it++) {
        const int zero = (it == 0 && !guess);
        if (alt && !(it & 1)) {                                 /* a y sweep from the state this sweep finds: mg_line.c's, one sweep */
            F->guess_nonzero = !zero;
            const int rc = mg_line_smooth(s, l, 1);
            F->guess_nonzero = guess;
            if (rc) return rc;
            continue;
        }
        if (L->xchunktab) {                                     /* mg_config.xline_chunk, a level with separators: mg_xline_chunk.c's four passes */
            F->guess_nonzero = !zero;
            const int rc = mg_xline_chunk_smooth(s, l, 1);
            F->guess_nonzero = guess;
            if (rc) return rc;
            continue;
        }
        const double *uin = zero ? NULL : u;
        CHK(mgk_xline_forward_f64(s->ctx, &F->g, L->ctab, L->xgtab, L->xgs, b, uin, z, NULL));
        CHK(mgk_xline_backward_f64(s->ctx, &F->g, L->ctab, L->xgtab, L->xgs, s->cfg.scale, z, uin, u, NULL));
    }
    return 0;
}
