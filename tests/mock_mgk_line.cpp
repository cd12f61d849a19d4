// mock_mgk_line.cpp -- host-memory stand-ins for the y-line Jacobi entry points (mgk_line_forward_f64, mgk_line_backward_f64) in the stated
// arithmetic (include/mgk.h): the five-term residual in the order of mgk_rowcoef_f64, one multiply and one subtract per row of the two
// recurrences, every product and sum rounded on its own (-ffp-contract=off), interior points only.  tests/mock_mgk.cpp's context and
// helpers are private to it, so it is included textually (and stays as it is).  Linked with mg_solver.c, mg_comm.c and mg_line.c by
// tests/test_line_cpu.py.  Like the other stand-ins they are recorded when a graph is being captured.  Every stand-in counts its executions.
#include "mock_mgk.cpp"

static int g_line_calls[2] = {0, 0};                // forward, backward
extern "C" int mock_line_calls(int which) { return (which >= 0 && which < 2) ? g_line_calls[which] : -1; }
extern "C" void mock_line_calls_reset(void) { g_line_calls[0] = g_line_calls[1] = 0; }

extern "C" {
int mgk_line_forward_f64(mgk_ctx *c, const mgk_geom *g, const double *atab, const double *ltab, const double *gtab, const double *b,
                         const double *u, double *z, void *) {
    if (!c || !g || g->dim != 2 || !ltab || !gtab || !b || !z || (u && !atab) || z == b || z == u) return fail(MGK_EINVAL, "mgk_line_forward_f64");
    const mgk_geom G = *g;
    return run(c, [=] {
        g_line_calls[0]++;
        for (int j = 0; j < G.nx; j++) {
            double y = 0.0;
            for (int i = 0; i < G.ny; i++) {
                double r = at(b, G, 0, i, j);
                if (u) {
                    const double *k = atab + 5 * (long)i;
                    double s = k[0] * at(u, G, 0, i - 1, j);
                    s = s + k[1] * at(u, G, 0, i, j - 1);
                    s = s + k[2] * at(u, G, 0, i, j);
                    s = s + k[3] * at(u, G, 0, i, j + 1);
                    s = s + k[4] * at(u, G, 0, i + 1, j);
                    r = r - s;
                }
                const double t = ltab[i] * y;
                y = r - t;
                at(z, G, 0, i, j) = y * gtab[i];
            }
        }
    });
}
int mgk_line_backward_f64(mgk_ctx *c, const mgk_geom *g, const double *qtab, double scale, const double *z, const double *u, double *unew, void *) {
    if (!c || !g || g->dim != 2 || !qtab || !z || !unew || unew == z) return fail(MGK_EINVAL, "mgk_line_backward_f64");
    const mgk_geom G = *g;
    return run(c, [=] {
        g_line_calls[1]++;
        for (int j = 0; j < G.nx; j++) {
            double e = 0.0;
            for (int i = G.ny - 1; i >= 0; i--) {
                const double t = qtab[i] * e;
                e = at(z, G, 0, i, j) - t;
                const double se = scale * e;
                at(unew, G, 0, i, j) = u ? at(u, G, 0, i, j) + se : se;
            }
        }
    });
}
}   // extern "C"
