/*
 * mg_xline_chunk.c -- the x-line sweeps in chunks (mg_config.xline_chunk = c, a multiple of 16, include/mgsolve.h):
 * mg_line_chunk.c turned by 90 degrees, a partitioned (separator / Schur complement) solve of the x-tridiagonal systems of mg_xline.c, so that
 * a pass runs on (K + 1) times as many waves.  K = n / c: column s_q = q c + c - 1 is separator q, the columns [k c, min(k c + c - 1, n)) are
 * chunk k (0 <= k <= K; the last one is empty when n = K c).  In grid row i the system is the constant-band matrix (W_i, C_i, E_i), so the
 * tables have `rows` = 1 row on the uniform mesh and n otherwise, as mg_xline.c's.  Computed here once per level (C99 double, no FMA:
 * -ffp-contract=off), one device array [g | v | w | SL SG SQ]:
 *
 *   g         mg_xline_factor's recurrence restarted in every chunk, a stored 0 in the separator columns (the multipliers l = W g_{j-1} and
 *             q = E g_j are one rounded product each, formed by the kernels and by chunk_solve below)
 *   v, w      the spikes T_k^-1 (W e_a) and T_k^-1 (E e_{b-1}) of chunk k = [a, b), by the two substitutions of the sweep on that right-hand
 *             side; v = 0 on chunk 0, w = 0 on chunk K, both 0 in the separator columns (stored zeros: the edge cases are exact)
 *   SL SG SQ  band_factor's recurrence (mg_line_factor.h) on the Schur rows d_q = (C - W w[s-1]) - E v[s+1], sub_q = -(W v[s-1]),
 *             sup_q = -(E w[s+1]) (s = n - 1: d_q = C - W w[s-1], sup_q = 0), per grid row; stored separator-major, entry [q sstride + i],
 *             so that a lane that owns a row reads them coalesced (sstride = 0 on the uniform mesh: one double per separator, entry [q])
 *
 * g, v and w lie at mg_xline_stride's row stride (n doubles rounded up to 16, the padding zero; 0 on the uniform mesh), each table a
 * whole number of 128-byte lines.  A sweep is four passes (include/mgk.h) over the level's tmp and a separator workspace of 4 K rows (the
 * planes R, XL, XR, XI), allocated here: forward and backward substitution in every chunk, the separator system, the correction and the update
 * in place in u.  No buffer is swapped.  A level with n < c has no separator: it keeps mg_xline.c's two passes on mg_xline.c's table.  This
 * file is the only host code that calls the four kernels; mg_solver.c and mg_xline.c refer to it weakly (mg_solver_internal.h).
 */
#include "mg_solver_internal.h"
#include "mg_line_factor.h"
#include <stdlib.h>

/* the two substitutions of the sweep on the columns [a, b) of x, in place: r -> x' */
static void chunk_solve(double W, double E, const double *g, int a, int b, double *x) {
    double y = x[a];
    x[a] = y * g[a];
    for (int j = a + 1; j < b; j++) {
        const double l = W * g[j - 1];
        const double t = l * y;
        y = x[j] - t;
        x[j] = y * g[j];
    }
    double e = x[b - 1];
    for (int j = b - 2; j >= a; j--) {
        const double q = E * g[j];
        const double t = q * e;
        e = x[j] - t;
        x[j] = e;
    }
}

/* the lengths of a level's tables: T doubles for each of g, v, w and KS for each of SL, SG, SQ */
static void table_lengths(const mg_solver *s, const mg_level *L, int K, size_t *T, size_t *KS, long *gs, long *ss) {
    const int uniform = (s->cfg.mesh == 0);
    *gs = mg_xline_stride(L->n, uniform);
    *ss = uniform ? 0 : (long)round16((size_t)L->n);
    *T = uniform ? round16((size_t)L->n) : (size_t)L->n * (size_t)*gs;
    *KS = uniform ? (size_t)K : (size_t)K * (size_t)*ss;
}

int mg_xline_chunk_tables(mg_solver *s, int lev, const double *ctab) {
    mg_level *L = &s->L[lev];
    const int n = L->n, c = s->cfg.xline_chunk, K = c > 0 ? n / c : 0;
    if (K < 1) return 0;                                        /* a short level: mg_xline.c's sweep */
    const int rows = (s->cfg.mesh == 0) ? 1 : n;
    size_t T, KS;
    long gs, ss;
    table_lengths(s, L, K, &T, &KS, &gs, &ss);
    const size_t len = 3 * T + 3 * KS;
    double *h = (double *)calloc(len + (size_t)n + 6 * (size_t)K, sizeof(double));
    if (!h) return mgi_fail(MGK_EINVAL, "mg_xline_chunk_tables: out of host memory");
    double *SLt = h + 3 * T, *SGt = SLt + KS, *SQt = SGt + KS;
    double *x = h + len, *sub = x + n, *dia = sub + K, *sup = dia + K, *fl = sup + K, *fg = fl + K, *fq = fg + K;    /* scratch */
    for (int i = 0; i < rows; i++) {
        const double *r = ctab + 5 * (size_t)i;
        const double W = r[1], Cc = r[2], E = r[3];
        double *g = h + (size_t)i * (size_t)gs, *v = g + T, *w = v + T;
        for (int k = 0; k <= K; k++) {
            const int a = k * c, b = (a + c - 1 < n) ? a + c - 1 : n;
            if (b <= a) continue;
            mg_xline_factor(b - a, 1, r, 0, g + a);
            if (k > 0) {
                for (int j = a; j < b; j++) x[j] = 0.0;
                x[a] = W;
                chunk_solve(W, E, g, a, b, x);
                for (int j = a; j < b; j++) v[j] = x[j];
            }
            if (k < K) {
                for (int j = a; j < b; j++) x[j] = 0.0;
                x[b - 1] = E;
                chunk_solve(W, E, g, a, b, x);
                for (int j = a; j < b; j++) w[j] = x[j];
            }
        }
        for (int q = 0; q < K; q++) {
            const int sc = q * c + c - 1;
            double t = W * w[sc - 1];
            dia[q] = Cc - t;
            t = W * v[sc - 1];
            sub[q] = -t;
            sup[q] = 0.0;
            if (sc < n - 1) {
                t = E * v[sc + 1];
                dia[q] = dia[q] - t;
                t = E * w[sc + 1];
                sup[q] = -t;
            }
        }
        band_factor(K, 1, sub, dia, sup, fl, fg, fq);
        for (int q = 0; q < K; q++) {
            const size_t at = ss ? (size_t)q * (size_t)ss + (size_t)i : (size_t)q;
            SLt[at] = fl[q]; SGt[at] = fg[q]; SQt[at] = fq[q];
        }
    }
    int rc = mgi_upload(s, h, len, &L->xchunktab);
    free(h);
    if (rc) return rc;
    void *sep = NULL;
    rc = mgk_malloc(s->ctx, &sep, sizeof(double) * 4 * (size_t)K * round16((size_t)n));
    if (rc) return mgi_fail(rc, "mg_xline_chunk_tables: the separator workspace");
    L->xchunksep = (double *)sep;
    return 0;
}

/* maxit x sweeps on a level that has separators, from the state F->guess_nonzero names: four passes per sweep */
int mg_xline_chunk_smooth(mg_solver *s, int lev, int maxit) {
    mg_level *L = &s->L[lev];
    mg_fset *F = &L->f[0];
    const int c = s->cfg.xline_chunk, K = L->n / c;
    size_t T, KS;
    long gs, ss;
    table_lengths(s, L, K, &T, &KS, &gs, &ss);
    const double *g = L->xchunktab, *v = g + T, *w = v + T, *SLt = w + T, *SGt = SLt + KS, *SQt = SGt + KS;
    const double *b = (const double *)F->b;
    double *u = (double *)F->u, *t = (double *)F->tmp, *sep = L->xchunksep;
    for (int it = 0; it < maxit; it++) {
        const double *uin = (it == 0 && !F->guess_nonzero) ? NULL : u;
        CHK(mgk_xline_chunk_forward_f64(s->ctx, &F->g, c, L->ctab, g, gs, b, uin, t, sep, NULL));
        CHK(mgk_xline_chunk_backward_f64(s->ctx, &F->g, c, L->ctab, g, gs, t, sep, NULL));
        CHK(mgk_xline_chunk_reduce_f64(s->ctx, &F->g, c, L->ctab, SLt, SGt, SQt, ss, sep, NULL));
        CHK(mgk_xline_chunk_correct_f64(s->ctx, &F->g, c, v, w, gs, s->cfg.scale, t, sep, uin, u, NULL));
    }
    return 0;
}
