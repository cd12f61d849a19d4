/*
 * mg_line_factor.h -- the host arithmetic the line smoothers' table builders share (mg_line.c, mg_xline.c, mg_line_chunk.c, mg_xline_chunk.c).
 * Private to libmgpetsc.so like mg_solver_internal.h; static inline functions only, so no host file depends on another through it.
 */
#ifndef MG_LINE_FACTOR_H
#define MG_LINE_FACTOR_H
#include <stddef.h>

/* n doubles rounded up to whole 128-byte lines */
static inline size_t round16(size_t n) { return (n + 15) / 16 * 16; }

/* The factorisation of a tridiagonal matrix given by three bands of n entries, entry i of a band at [i * st] (C99 double, no FMA:
 * -ffp-contract=off):  m_0 = dia_0, g_0 = 1/m_0, l_0 = 0;   i >= 1: l_i = sub_i g_{i-1}, t = l_i sup_{i-1}, m_i = dia_i - t, g_i = 1/m_i;
 * q_i = sup_i g_i.  The tables lt, gt, qt are contiguous. */
static inline void band_factor(int n, size_t st, const double *sub, const double *dia, const double *sup, double *lt, double *gt, double *qt) {
    if (n < 1) return;
    double m = dia[0];
    gt[0] = 1.0 / m;
    lt[0] = 0.0;
    for (int i = 1; i < n; i++) {
        lt[i] = sub[i * st] * gt[i - 1];
        const double t = lt[i] * sup[(i - 1) * st];
        m = dia[i * st] - t;
        gt[i] = 1.0 / m;
    }
    for (int i = 0; i < n; i++) qt[i] = sup[i * st] * gt[i];
}
#endif
