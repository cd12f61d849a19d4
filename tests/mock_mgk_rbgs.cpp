// mock_mgk_rbgs.cpp -- host-memory stand-ins for the red-black Gauss-Seidel entry points (mgk_rbgs_2d_f64, mgk_prolong_rbgs_2d_f64) in the stated
// arithmetic (include/mgk.h): colour (i + j) & 1, a half-sweep of colour 0, then of colour 1, each point by u + scale * ((b - t) * dinv) with
// the five-term sum t in the order of mgk_rowcoef_f64 over the field the half-sweep started from, every product and sum rounded on its own
// (-ffp-contract=off); ghosts count as zeros, interior points only are written.  tests/mock_mgk.cpp's context and helpers are private to it,
// so it is included textually (and stays as it is).  Linked with mg_solver.c, mg_comm.c and mg_rbgs.c by tests/test_rbgs_cpu.py.  Like the
// other stand-ins they are recorded when a graph is being captured.  Every stand-in counts its executions.  The stand-ins that csrc/mg_fmg.c
// and csrc/mg_gmres.c name come along (tests/mock_mgk_fmg.cpp; mock_mgk.cpp guards itself against the second inclusion), so that fmg,
// solve_fmg and solve_gmres on a red-black handle exist and are REFUSED by the product's own checks.
#include "mock_mgk.cpp"
#include "mock_mgk_fmg.cpp"

static int g_rbgs_calls[3] = {0, 0, 0};             // plain, zero guess, with prolongation
extern "C" int mock_rbgs_calls(int which) { return (which >= 0 && which < 3) ? g_rbgs_calls[which] : -1; }
extern "C" void mock_rbgs_calls_reset(void) { g_rbgs_calls[0] = g_rbgs_calls[1] = g_rbgs_calls[2] = 0; }

// nsweeps sweeps on the compact copy `cur` (ny x nx) of the field; the result goes to the interior of out
static void rbgs_run(const mgk_geom &G, const std::vector<double> &coef, double dinv_, double scale, const double *ctab, const double *dtab, int nsweeps,
                     const double *b, std::vector<double> cur, double *out) {
    const int nx = G.nx, ny = G.ny;
    auto get = [&](const std::vector<double> &f, int i, int j) -> double { return (i < 0 || i >= ny || j < 0 || j >= nx) ? 0.0 : f[(size_t)i * nx + j]; };
    for (int st = 0; st < 2 * nsweeps; st++) {
        std::vector<double> nxt = cur;
        for (int i = 0; i < ny; i++) {
            const double *k = ctab ? ctab + 5 * (long)i : coef.data();
            const double dinv = ctab ? dtab[i] : dinv_;
            for (int j = 0; j < nx; j++) {
                if (((i + j) & 1) != (st & 1)) continue;
                double s = k[0] * get(cur, i - 1, j);
                s = s + k[1] * get(cur, i, j - 1);
                s = s + k[2] * get(cur, i, j);
                s = s + k[3] * get(cur, i, j + 1);
                s = s + k[4] * get(cur, i + 1, j);
                const double res = at(b, G, 0, i, j) - s;
                const double zz = res * dinv;
                nxt[(size_t)i * nx + j] = get(cur, i, j) + scale * zz;
            }
        }
        cur.swap(nxt);
    }
    for (int i = 0; i < ny; i++) for (int j = 0; j < nx; j++) at(out, G, 0, i, j) = cur[(size_t)i * nx + j];
}
static bool rbgs_args_ok(mgk_ctx *c, const mgk_geom *g, const double *coef, const double *ctab, const double *dtab, int nsweeps, const double *b, const double *u,
                         const double *unew) {
    return c && g && g->dim == 2 && (coef || ctab) && (!ctab || dtab) && b && unew && unew != u && unew != b && (nsweeps == 1 || nsweeps == 2);
}

extern "C" {
int mgk_rbgs_2d_f64(mgk_ctx *c, const mgk_geom *g, const double *coef, double dinv, double scale, const double *ctab, const double *dtab, int nsweeps,
                    const double *b, const double *u, double *unew, void *) {
    if (!rbgs_args_ok(c, g, coef, ctab, dtab, nsweeps, b, u, unew)) return fail(MGK_EINVAL, "mgk_rbgs_2d_f64");
    const mgk_geom G = *g;
    std::vector<double> k(5, 0.0);
    if (coef) k.assign(coef, coef + 5);
    return run(c, [=] {
        g_rbgs_calls[u ? 0 : 1]++;
        std::vector<double> cur((size_t)G.nx * G.ny, 0.0);
        if (u) for (int i = 0; i < G.ny; i++) for (int j = 0; j < G.nx; j++) cur[(size_t)i * G.nx + j] = at(u, G, 0, i, j);
        rbgs_run(G, k, dinv, scale, ctab, dtab, nsweeps, b, cur, unew);
    });
}
int mgk_prolong_rbgs_2d_f64(mgk_ctx *c, const mgk_geom *gf, const mgk_geom *gc, const double *coef, double dinv, double scale, const double *ctab,
                            const double *dtab, int nsweeps, const double *b, const double *uc, const double *u, double *unew, void *) {
    if (!rbgs_args_ok(c, gf, coef, ctab, dtab, nsweeps, b, u, unew) || !u || !uc || !xfer_ok(gf, gc)) return fail(MGK_EINVAL, "mgk_prolong_rbgs_2d_f64");
    const mgk_geom F = *gf, Cg = *gc;
    std::vector<double> k(5, 0.0);
    if (coef) k.assign(coef, coef + 5);
    return run(c, [=] {
        g_rbgs_calls[2]++;
        std::vector<double> cur((size_t)F.nx * F.ny);
        for (int i = 0; i < F.ny; i++) for (int j = 0; j < F.nx; j++)       // the arithmetic of mgk_prolong_add_f64
            cur[(size_t)i * F.nx + j] = at(u, F, 0, i, j) + prolong_at(F, Cg, uc, 1, i, j);
        rbgs_run(F, k, dinv, scale, ctab, dtab, nsweeps, b, cur, unew);
    });
}
}   // extern "C"
