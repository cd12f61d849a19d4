/*
 * mg_line_chunk.c -- the y-line sweeps in chunks (mg_config.line_chunk = c >= 2, include/mgsolve.h): a partitioned
 * (separator / Schur complement) solve of the y-tridiagonal systems of mg_line.c, so that a pass runs on (K + 1) times as many waves.
 * Period c, K = n / c: row s_j = j c + c - 1 is separator j, the rows [k c, min(k c + c - 1, n)) are chunk k (0 <= k <= K; the last one is
 * empty when n = K c).  Tables per level, computed here once (C99 double, no FMA: -ffp-contract=off), one device array [l g q v w | L G Q]:
 *
 *   l, g, q   band_factor (mg_line_factor.h), mg_line.c's factorisation, restarted in every chunk (l_a = 0, m_a = C_a), 0 in the separator rows
 *   v, w      the spikes T_k^-1 (S_a e_a) and T_k^-1 (N_{b-1} e_{b-1}) of chunk k = [a, b), by the two substitutions of the sweep on that
 *             right-hand side; v = 0 on chunk 0, w = 0 on the last chunk, both 0 in the separator rows (stored zeros: the edge cases are exact)
 *   L, G, Q   band_factor's recurrence on the Schur rows d_j = (C_s - S_s w[s-1]) - N_s v[s+1], sub_j = -(S_s v[s-1]), sup_j = -(N_s w[s+1])
 *             (s = n - 1: d_j = C_s - S_s w[s-1], sup_j = 0)
 *
 * A sweep is four passes (include/mgk.h): forward and backward substitution in every chunk (z, then x' in the level's tmp, the residual r_s
 * in the separator rows), the separator system (xi_j into the separator rows), the correction and the update in place in u.  No buffer is
 * swapped, as in mg_line.c.  A level with n < c has no separator: it keeps mg_line.c's two passes on mg_line.c's tables.  This file is the
 * only host code that calls the four kernels; mg_solver.c and mg_line.c refer to it weakly (mg_solver_internal.h).
 */
#include "mg_solver_internal.h"
#include "mg_line_factor.h"
#include <stdlib.h>

/* the two substitutions of the sweep on the rows [a, b) of x, in place: r -> x' */
static void chunk_solve(const double *l, const double *g, const double *q, int a, int b, double *x) {
    double y = x[a];
    x[a] = y * g[a];
    for (int i = a + 1; i < b; i++) {
        const double t = l[i] * y;
        y = x[i] - t;
        x[i] = y * g[i];
    }
    double e = x[b - 1];
    for (int i = b - 2; i >= a; i--) {
        const double t = q[i] * e;
        e = x[i] - t;
        x[i] = e;
    }
}

int mg_line_chunk_tables(mg_solver *s, int lev, const double *ctab) {
    mg_level *L = &s->L[lev];
    const int n = L->n, c = s->cfg.line_chunk, K = c >= 2 ? n / c : 0;
    if (K < 1) return 0;                                        /* a short level: mg_line.c's sweep */
    const size_t N = (size_t)n, len = 5 * N + 3 * (size_t)K;
    double *h = (double *)calloc(len + 4 * N + 3 * (size_t)K, sizeof(double));
    if (!h) return mgi_fail(MGK_EINVAL, "mg_line_chunk_tables: out of host memory");
    double *l = h, *g = h + N, *q = h + 2 * N, *v = h + 3 * N, *w = h + 4 * N, *LL = h + 5 * N, *GG = LL + K, *QQ = GG + K;
    double *x = h + len, *bs = x + N, *bd = bs + N, *bu = bd + N;   /* scratch: a right-hand side; the three bands of a chunk */
    double *sub = bu + N, *dia = sub + K, *sup = dia + K;           /* ... and the Schur rows */
    for (int k = 0; k <= K; k++) {
        const int a = k * c, b = (a + c - 1 < n) ? a + c - 1 : n;
        if (b <= a) continue;
        for (int i = a; i < b; i++) { bs[i] = ctab[5 * (size_t)i]; bd[i] = ctab[5 * (size_t)i + 2]; bu[i] = ctab[5 * (size_t)i + 4]; }
        band_factor(b - a, 1, bs + a, bd + a, bu + a, l + a, g + a, q + a);
        if (k > 0) {
            for (int i = a; i < b; i++) x[i] = 0.0;
            x[a] = bs[a];
            chunk_solve(l, g, q, a, b, x);
            for (int i = a; i < b; i++) v[i] = x[i];
        }
        if (k < K) {
            for (int i = a; i < b; i++) x[i] = 0.0;
            x[b - 1] = bu[b - 1];
            chunk_solve(l, g, q, a, b, x);
            for (int i = a; i < b; i++) w[i] = x[i];
        }
    }
    for (int j = 0; j < K; j++) {
        const int r = j * c + c - 1;
        const double *row = ctab + 5 * (size_t)r;
        double t = row[0] * w[r - 1];
        dia[j] = row[2] - t;
        t = row[0] * v[r - 1];
        sub[j] = -t;
        sup[j] = 0.0;
        if (r < n - 1) {
            t = row[4] * v[r + 1];
            dia[j] = dia[j] - t;
            t = row[4] * w[r + 1];
            sup[j] = -t;
        }
    }
    band_factor(K, 1, sub, dia, sup, LL, GG, QQ);
    const int rc = mgi_upload(s, h, len, &L->chunktab);
    free(h);
    return rc;
}

/* mg_line_smooth's loop on a level that has separators: four passes per sweep */
int mg_line_chunk_smooth(mg_solver *s, int lev, int maxit) {
    mg_level *L = &s->L[lev];
    mg_fset *F = &L->f[0];
    const int c = s->cfg.line_chunk;
    const size_t n = (size_t)L->n;
    const double *T = L->chunktab, *TL = T + 5 * n, *TG = TL + L->n / c, *TQ = TG + L->n / c;
    const double *b = (const double *)F->b;
    double *u = (double *)F->u, *z = (double *)F->tmp;
    if (maxit == 0 && !F->guess_nonzero) CHK(mgk_memset0(s->ctx, u, sizeof(double) * (size_t)F->g.total, NULL));   /* KSPSolve zero-fills */
    for (int it = 0; it < maxit; it++) {
        const double *uin = (it == 0 && !F->guess_nonzero) ? NULL : u;
        CHK(mgk_line_chunk_forward_f64(s->ctx, &F->g, c, L->ctab, T, T + n, b, uin, z, NULL));
        CHK(mgk_line_chunk_backward_f64(s->ctx, &F->g, c, T + 2 * n, z, NULL));
        CHK(mgk_line_chunk_reduce_f64(s->ctx, &F->g, c, L->ctab, TL, TG, TQ, z, NULL));
        CHK(mgk_line_chunk_correct_f64(s->ctx, &F->g, c, T + 3 * n, T + 4 * n, s->cfg.scale, z, uin, u, NULL));
    }
    return 0;
}
