// mock_mgk_xline.cpp -- host-memory stand-ins for the x-line Jacobi entry points (mgk_xline_forward_f64, mgk_xline_backward_f64) in the
// stated arithmetic (include/mgk.h): the five-term residual in the order of mgk_rowcoef_f64, the multipliers l = W g and q = E g one rounded
// product each, one multiply and one subtract per column of the two recurrences, every product and sum rounded on its own
// (-ffp-contract=off), interior points only.  tests/mock_mgk_line.cpp (and with it tests/mock_mgk.cpp) is included textually and stays as it
// is.  Linked with mg_solver.c, mg_comm.c, mg_line.c and mg_xline.c by tests/test_xline_cpu.py.  Every stand-in of a line pass, y or x,
// appends a letter to a log when it EXECUTES (f / b: the y passes, F / B: the x passes), so that the order of the sweeps shows.
#include "mock_mgk_line.cpp"
#include <string>

static std::string g_xline_log;
// the y stand-ins only count their executions (g_line_calls): the log is brought up to date from the counters before every x pass and when
// it is read.  A y sweep is a forward pass followed by its backward pass, so the counters advance in pairs
static int g_seen[2] = {0, 0};
static void note_y() {
    while (g_seen[0] < g_line_calls[0] || g_seen[1] < g_line_calls[1]) {
        if (g_seen[0] < g_line_calls[0]) { g_xline_log += 'f'; g_seen[0]++; }
        if (g_seen[1] < g_line_calls[1]) { g_xline_log += 'b'; g_seen[1]++; }
    }
}
extern "C" const char *mock_xline_log(void) { note_y(); return g_xline_log.c_str(); }
extern "C" void mock_xline_log_clear(void) { g_xline_log.clear(); mock_line_calls_reset(); g_seen[0] = g_seen[1] = 0; }

extern "C" {
int mgk_xline_forward_f64(mgk_ctx *c, const mgk_geom *g, const double *atab, const double *gtab, long gs, const double *b, const double *u,
                          double *z, void *) {
    if (!c || !g || g->dim != 2 || !atab || !gtab || !b || !z || z == b || z == u || (gs != 0 && gs < g->nx)) return fail(MGK_EINVAL, "mgk_xline_forward_f64");
    const mgk_geom G = *g;
    return run(c, [=] {
        note_y();
        g_xline_log += 'F';
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
                if (j == 0) y = r;
                else {
                    const double l = k[1] * gi[j - 1];
                    const double t = l * y;
                    y = r - t;
                }
                at(z, G, 0, i, j) = y * gi[j];
            }
        }
    });
}
int mgk_xline_backward_f64(mgk_ctx *c, const mgk_geom *g, const double *atab, const double *gtab, long gs, double scale, const double *z,
                           const double *u, double *unew, void *) {
    if (!c || !g || g->dim != 2 || !atab || !gtab || !z || !unew || unew == z || (gs != 0 && gs < g->nx)) return fail(MGK_EINVAL, "mgk_xline_backward_f64");
    const mgk_geom G = *g;
    return run(c, [=] {
        note_y();
        g_xline_log += 'B';
        for (int i = 0; i < G.ny; i++) {
            const double *k = atab + 5 * (long)i, *gi = gtab + (long)i * gs;
            double e = 0.0;
            for (int j = G.nx - 1; j >= 0; j--) {
                if (j == G.nx - 1) e = at(z, G, 0, i, j);
                else {
                    const double q = k[3] * gi[j];
                    const double t = q * e;
                    e = at(z, G, 0, i, j) - t;
                }
                const double se = scale * e;
                at(unew, G, 0, i, j) = u ? at(u, G, 0, i, j) + se : se;
            }
        }
    });
}
}   // extern "C"
