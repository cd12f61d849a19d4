// mock_mgk_xchunkline.cpp -- host-memory stand-ins for the four passes of the x-line sweep in chunks (mgk_xline_chunk_forward_f64, _backward_,
// _reduce_, _correct_) in the stated arithmetic (include/mgk.h): every product and sum rounded on its own
// (-ffp-contract=off), interior points only, the separator workspace as the kernels lay it out (four planes R, XL, XR, XI of K rows of
// ny rounded up to 16 doubles), an entry the definition never forms neither written nor read.  tests/mock_mgk_chunkline.cpp is included
// textually and stays as it is (and through it the stand-ins of the plain y and x passes and of the chunked y passes: a level without
// separators runs the plain stand-ins, altline with both options set all of them).  Linked with mg_solver.c, mg_comm.c, mg_line.c,
// mg_xline.c, mg_line_chunk.c and mg_xline_chunk.c by tests/test_xchunkline_cpu.py.  Recorded when a graph is being captured, like the other
// stand-ins.  Every stand-in counts its executions; the plain x passes are counted from the log of tests/mock_mgk_xline.cpp.
#include "mock_mgk_chunkline.cpp"    // (includes mock_mgk_xline.cpp, mock_mgk_line.cpp and mock_mgk.cpp)

static int g_xchunk_calls[4] = {0, 0, 0, 0};        // forward, backward, reduce, correct
extern "C" int mock_xchunk_calls(int which) { return (which >= 0 && which < 4) ? g_xchunk_calls[which] : -1; }
extern "C" void mock_xchunk_calls_reset(void) { g_xchunk_calls[0] = g_xchunk_calls[1] = g_xchunk_calls[2] = g_xchunk_calls[3] = 0; }
static inline int xchunk_end(int k, int c, int n) { return k * c + c - 1 < n ? k * c + c - 1 : n; }
static inline bool xchunk_ok(const mgk_geom *g, int cc, long stride) { return g && g->dim == 2 && cc > 0 && cc % 16 == 0 && stride >= 0 && stride <= (1L << 21); }
static inline long xchunk_ss(const mgk_geom &G) { return ((long)G.ny + 15) / 16 * 16; }

extern "C" {
int mgk_xline_chunk_forward_f64(mgk_ctx *c, const mgk_geom *g, int cc, const double *atab, const double *gtab, long gs, const double *b,
                                const double *u, double *t, double *sep, void *) {
    if (!c || !xchunk_ok(g, cc, gs) || (gs != 0 && gs < g->nx) || !atab || !gtab || !b || !t || t == b || t == u || t == sep || (g->nx >= cc && !sep))
        return fail(MGK_EINVAL, "mgk_xline_chunk_forward_f64");
    const mgk_geom G = *g;
    return run(c, [=] {
        g_xchunk_calls[0]++;
        const int K = G.nx / cc;
        const long ss = xchunk_ss(G);
        for (int i = 0; i < G.ny; i++) {
            const double *k = atab + 5 * (long)i, *gi = gtab + (long)i * gs;
            double y = 0.0;
            for (int j = 0; j < G.nx; j++) {
                double r = at(b, G, 0, i, j);
                if (u) {
                    double s = k[0] * at(u, G, 0, i - 1, j);
                    s = s + k[1] * at(u, G, 0, i, j - 1);
                    s = s + k[2] * at(u, G, 0, i, j);
                    s = s + k[3] * at(u, G, 0, i, j + 1);
                    s = s + k[4] * at(u, G, 0, i + 1, j);
                    r = r - s;
                }
                if (j % cc == cc - 1 && j / cc < K) {           // a separator column keeps its residual
                    at(t, G, 0, i, j) = r;
                    sep[(long)(j / cc) * ss + i] = r;
                    continue;
                }
                if (j % cc == 0) y = r;
                else {
                    const double l = k[1] * gi[j - 1];
                    const double p = l * y;
                    y = r - p;
                }
                at(t, G, 0, i, j) = y * gi[j];
            }
        }
    });
}
int mgk_xline_chunk_backward_f64(mgk_ctx *c, const mgk_geom *g, int cc, const double *atab, const double *gtab, long gs, double *t, double *sep,
                                 void *) {
    if (!c || !xchunk_ok(g, cc, gs) || (gs != 0 && gs < g->nx) || !atab || !gtab || !t || t == sep || (g->nx >= cc && !sep))
        return fail(MGK_EINVAL, "mgk_xline_chunk_backward_f64");
    const mgk_geom G = *g;
    return run(c, [=] {
        g_xchunk_calls[1]++;
        const int K = G.nx / cc;
        const long ss = xchunk_ss(G);
        for (int i = 0; i < G.ny; i++) {
            const double *k = atab + 5 * (long)i, *gi = gtab + (long)i * gs;
            for (int q = 0; q <= K; q++) {
                const int a = q * cc, e = xchunk_end(q, cc, G.nx);
                if (e <= a) continue;
                double x = at(t, G, 0, i, e - 1);
                for (int j = e - 2; j >= a; j--) {
                    const double m = k[3] * gi[j];
                    const double p = m * x;
                    x = at(t, G, 0, i, j) - p;
                    at(t, G, 0, i, j) = x;
                }
                if (q < K) sep[((long)K + q) * ss + i] = at(t, G, 0, i, e - 1);
                if (q > 0) sep[(2L * K + q - 1) * ss + i] = at(t, G, 0, i, a);
            }
        }
    });
}
int mgk_xline_chunk_reduce_f64(mgk_ctx *c, const mgk_geom *g, int cc, const double *atab, const double *SLt, const double *SGt, const double *SQt,
                               long sst, double *sep, void *) {
    if (!c || !xchunk_ok(g, cc, sst) || (sst != 0 && sst < g->ny) || (g->nx >= cc && (!atab || !SLt || !SGt || !SQt || !sep)))
        return fail(MGK_EINVAL, "mgk_xline_chunk_reduce_f64");
    const mgk_geom G = *g;
    return run(c, [=] {
        g_xchunk_calls[2]++;
        const int K = G.nx / cc;
        const long ss = xchunk_ss(G);
        double *R = sep, *XL = sep + (long)K * ss, *XR = XL + (long)K * ss, *XI = XR + (long)K * ss;
        for (int i = 0; i < G.ny; i++) {
            const double *k = atab + 5 * (long)i;
            const long ti = sst ? i : 0, qs = sst ? sst : 1;      // sstride 0: entry [q] for every row
            double Y = 0.0;
            for (int q = 0; q < K; q++) {
                const int s = q * cc + cc - 1;
                double p = k[1] * XL[q * ss + i];
                double rho = R[q * ss + i] - p;
                if (s < G.nx - 1) {
                    p = k[3] * XR[q * ss + i];
                    rho = rho - p;
                }
                if (q == 0) Y = rho;
                else {
                    p = SLt[q * qs + ti] * Y;
                    Y = rho - p;
                }
                XI[q * ss + i] = Y * SGt[q * qs + ti];
            }
            for (int q = K - 2; q >= 0; q--) {
                const double p = SQt[q * qs + ti] * XI[(q + 1) * ss + i];
                XI[q * ss + i] = XI[q * ss + i] - p;
            }
        }
    });
}
int mgk_xline_chunk_correct_f64(mgk_ctx *c, const mgk_geom *g, int cc, const double *vtab, const double *wtab, long gs, double scale, const double *t,
                                const double *sep, const double *u, double *unew, void *) {
    if (!c || !xchunk_ok(g, cc, gs) || (gs != 0 && gs < g->nx) || (gs & 1) || !t || !unew || unew == t || t == sep || (g->nx >= cc && (!vtab || !wtab || !sep)))
        return fail(MGK_EINVAL, "mgk_xline_chunk_correct_f64");
    const mgk_geom G = *g;
    return run(c, [=] {
        g_xchunk_calls[3]++;
        const int K = G.nx / cc;
        const long ss = xchunk_ss(G);
        const double *XI = sep + 3L * K * ss;
        for (int i = 0; i < G.ny; i++)
            for (int j = 0; j < G.nx; j++) {
                const int k = j / cc;
                double x = at(t, G, 0, i, j);
                if (j % cc == cc - 1 && k < K) x = XI[(long)k * ss + i];
                else {
                    if (k > 0) {
                        const double p = XI[(long)(k - 1) * ss + i] * vtab[(long)i * gs + j];
                        x = x - p;
                    }
                    if (k < K) {
                        const double p = XI[(long)k * ss + i] * wtab[(long)i * gs + j];
                        x = x - p;
                    }
                }
                const double se = scale * x;
                at(unew, G, 0, i, j) = u ? at(u, G, 0, i, j) + se : se;
            }
    });
}
}   // extern "C"
