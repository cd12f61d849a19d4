// mock_mgk_cg.cpp -- host-memory stand-ins for the entry points of include/mgk_cg.h (mgk_cg_direction_apply_dot_f64, mgk_cg_update_sumsq_f64 and
// their reduction workspace) in the stated arithmetic: interior points only, p_new = z + (beta * p_old), A in the canonical order with every
// product and sum rounded separately, x + (alpha * p), r - (alpha * q); the sums in long double like the other reductions of mock_mgk.cpp.
// tests/mock_mgk_gmres.cpp (mgk_multi_dot_f64 among others, and through it tests/mock_mgk.cpp) is included textually and stays as it is; its
// mgk_malloc is renamed on the way in, so that the one defined here can be told to fail: mock_cg_fail_malloc(n) makes the n-th allocation
// from now on fail once (the path of mg_solver_solve_cg that must leave nothing allocated).  Linked with mg_solver.c, mg_comm.c, mg_cg.c,
// and mg_gmres.c by tests/test_cg_cpu.py.  The two passes count their calls; mock_cg_calls(2) gives the calls of mgk_multi_dot_f64, which the CG
// driver makes once per application of M (rho = r . z).
#define mgk_malloc mock_base_mgk_malloc
#include "mock_mgk_gmres.cpp"
#undef mgk_malloc
#include "mgk_cg.h"

struct mgk_cg_ws { double slots[16]; int nslots; };

static int g_cg_calls[3] = {0, 0, 0};               // direction, update, live workspaces
static long g_cg_fail_in = 0;
extern "C" int mock_cg_calls(int which) { return which == 2 ? g_kry_calls[0] : (which >= 0 && which < 2) ? g_cg_calls[which] : -1; }
extern "C" void mock_cg_calls_reset(void) { g_cg_calls[0] = g_cg_calls[1] = 0; mock_gmres_calls_reset(); }
extern "C" void mock_cg_fail_malloc(long nth) { g_cg_fail_in = nth; }
extern "C" int mock_cg_live_allocations(void) { return g_cg_calls[2]; }

extern "C" {
int mgk_malloc(mgk_ctx *c, void **p, size_t bytes) {
    if (g_cg_fail_in > 0 && --g_cg_fail_in == 0) { *p = nullptr; return fail(MGK_EINVAL, "mgk_malloc: told to fail"); }
    return mock_base_mgk_malloc(c, p, bytes);
}

int mgk_cg_workspace_create(mgk_ctx *c, mgk_cg_ws **out) {
    if (!c || !out) return fail(MGK_EINVAL, "mgk_cg_workspace_create");
    *out = new mgk_cg_ws();
    (*out)->nslots = 16;
    g_cg_calls[2]++;
    return 0;
}
void mgk_cg_workspace_destroy(mgk_ctx *c, mgk_cg_ws *ws) { if (c && ws) { delete ws; g_cg_calls[2]--; } }
int mgk_cg_workspace_debug(mgk_cg_ws *ws, double **parts, int *n) {
    if (!ws || !parts || !n) return fail(MGK_EINVAL, "mgk_cg_workspace_debug");
    *parts = ws->slots; *n = ws->nslots;
    return 0;
}

int mgk_cg_direction_apply_dot_f64(mgk_ctx *c, const mgk_geom *g, const double *coef, double beta, const double *z, const double *p_old,
                                   double *p_new, double *q, mgk_cg_ws *ws, double *sigma_host, void *) {
    if (!c || !g || !coef || !z || !p_new || !q || !ws) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: null argument");
    if (c->capturing) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: the stream is being captured");
    if (p_new == p_old || p_new == z || q == z || q == p_old || q == p_new) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: aliasing");
    g_cg_calls[0]++;
    const int d3 = g->dim == 3;
    KRY_INTERIOR(g) {
        double v = at(z, *g, kk, i, j);
        if (p_old) { const double t = beta * at(p_old, *g, kk, i, j); v = v + t; }
        at(p_new, *g, kk, i, j) = v;
    }
    long double s = 0;
    KRY_INTERIOR(g) {                                                   // (the ghost ring of p_new is zero: the driver's fields come zero-filled)
        const double *cf = coef;
        double t;
        if (d3) {
            t = cf[0] * at(p_new, *g, kk - 1, i, j);
            t = t + cf[1] * at(p_new, *g, kk, i - 1, j);
            t = t + cf[2] * at(p_new, *g, kk, i, j - 1);
            t = t + cf[3] * at(p_new, *g, kk, i, j);
            t = t + cf[4] * at(p_new, *g, kk, i, j + 1);
            t = t + cf[5] * at(p_new, *g, kk, i + 1, j);
            t = t + cf[6] * at(p_new, *g, kk + 1, i, j);
        } else {
            t = cf[0] * at(p_new, *g, kk, i - 1, j);
            t = t + cf[1] * at(p_new, *g, kk, i, j - 1);
            t = t + cf[2] * at(p_new, *g, kk, i, j);
            t = t + cf[3] * at(p_new, *g, kk, i, j + 1);
            t = t + cf[4] * at(p_new, *g, kk, i + 1, j);
        }
        at(q, *g, kk, i, j) = t;
        s += (long double)(at(p_new, *g, kk, i, j) * t);
    }
    ws->slots[0] = (double)s;
    if (sigma_host) *sigma_host = (double)s;
    return 0;
}

int mgk_cg_update_sumsq_f64(mgk_ctx *c, const mgk_geom *g, double alpha, const double *p, const double *q, double *x, double *r,
                            mgk_cg_ws *ws, double *sumsq_host, void *) {
    if (!c || !g || !p || !q || !x || !r || !ws) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64: null argument");
    if (c->capturing) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64: the stream is being captured");
    if (p == q || p == x || p == r || q == x || q == r || x == r) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64: aliasing");
    g_cg_calls[1]++;
    long double s = 0;
    KRY_INTERIOR(g) {
        const double tp = alpha * at(p, *g, kk, i, j), tq = alpha * at(q, *g, kk, i, j);
        at(x, *g, kk, i, j) = at(x, *g, kk, i, j) + tp;
        const double rr = at(r, *g, kk, i, j) - tq;
        at(r, *g, kk, i, j) = rr;
        s += (long double)(rr * rr);
    }
    ws->slots[1] = (double)s;
    if (sumsq_host) *sumsq_host = (double)s;
    return 0;
}
}   // extern "C"
