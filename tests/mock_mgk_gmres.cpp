// mock_mgk_gmres.cpp -- host-memory stand-ins for the Krylov entry points (mgk_multi_dot_f64, mgk_multi_axpy_sumsq_f64, mgk_krylov_fetch,
// mgk_lincomb_f64, mgk_scale_to_f64) in the stated arithmetic: interior points only, ascending i, multiply and add / subtract rounded
// separately; the sums in long double like the other reductions of mock_mgk.cpp.  That file's context and helpers are private to it, so it
// is included textually (and stays as it is).  Linked with mg_solver.c, mg_comm.c and mg_gmres.c by tests/test_gmres_cpu.py.  The reduced
// values go to `device` memory and to a landing area that mgk_krylov_fetch reads, as on the GPU.  Every stand-in counts its calls.
#include "mock_mgk.cpp"

static double g_kry_landing[MGK_KRYLOV_MAX + 1];
static int g_kry_calls[5] = {0, 0, 0, 0, 0};        // multi_dot, multi_axpy_sumsq, fetch, lincomb, scale_to
extern "C" int mock_gmres_calls(int which) { return (which >= 0 && which < 5) ? g_kry_calls[which] : -1; }
extern "C" void mock_gmres_calls_reset(void) { for (int q = 0; q < 5; q++) g_kry_calls[q] = 0; }

static bool kry_ok(mgk_ctx *c, const mgk_geom *g, int k, const double *const *v) {
    if (!c || c->capturing || !g || k < 1 || k > MGK_KRYLOV_MAX || !v) return false;
    for (int i = 0; i < k; i++) if (!v[i]) return false;
    return true;
}
#define KRY_INTERIOR(g) for (int kk = 0; kk < ((g)->dim == 3 ? (g)->nz : 1); kk++) for (int i = 0; i < (g)->ny; i++) for (int j = 0; j < (g)->nx; j++)

extern "C" {
int mgk_multi_dot_f64(mgk_ctx *c, const mgk_geom *g, int k, const double *const *v, const double *w, double *out_dev, double *out_host, void *) {
    if (!kry_ok(c, g, k, v) || !w || !out_dev) return fail(MGK_EINVAL, "mgk_multi_dot_f64");
    g_kry_calls[0]++;
    for (int q = 0; q < k; q++) {
        long double s = 0;
        KRY_INTERIOR(g) s += (long double)(at(v[q], *g, kk, i, j) * at(w, *g, kk, i, j));
        out_dev[q] = (double)s;
        g_kry_landing[q] = (double)s;
        if (out_host) out_host[q] = (double)s;
    }
    return 0;
}
int mgk_multi_axpy_sumsq_f64(mgk_ctx *c, const mgk_geom *g, int k, const double *h_dev, const double *const *v, double *w, double *sumsq_host, void *) {
    if (!kry_ok(c, g, k, v) || !h_dev || !w) return fail(MGK_EINVAL, "mgk_multi_axpy_sumsq_f64");
    for (int q = 0; q < k; q++) if (v[q] == w) return fail(MGK_EINVAL, "mgk_multi_axpy_sumsq_f64: w is one of the operands");
    g_kry_calls[1]++;
    long double s = 0;
    KRY_INTERIOR(g) {
        double x = at(w, *g, kk, i, j);
        for (int q = 0; q < k; q++) { const double t = h_dev[q] * at(v[q], *g, kk, i, j); x = x - t; }
        at(w, *g, kk, i, j) = x;
        s += (long double)(x * x);
    }
    g_kry_landing[MGK_KRYLOV_MAX] = (double)s;
    if (sumsq_host) *sumsq_host = (double)s;
    return 0;
}
int mgk_krylov_fetch(mgk_ctx *c, int k, double *h_host, double *sumsq_host, void *) {
    if (!c || k < 0 || k > MGK_KRYLOV_MAX || (k > 0 && !h_host)) return fail(MGK_EINVAL, "mgk_krylov_fetch");
    g_kry_calls[2]++;
    for (int q = 0; q < k; q++) h_host[q] = g_kry_landing[q];
    if (sumsq_host) *sumsq_host = g_kry_landing[MGK_KRYLOV_MAX];
    return 0;
}
int mgk_lincomb_f64(mgk_ctx *c, const mgk_geom *g, int k, const double *y, const double *const *v, double *out, void *) {
    if (!kry_ok(c, g, k, v) || !y || !out) return fail(MGK_EINVAL, "mgk_lincomb_f64");
    for (int q = 0; q < k; q++) if (v[q] == out) return fail(MGK_EINVAL, "mgk_lincomb_f64: out is one of the operands");
    g_kry_calls[3]++;
    KRY_INTERIOR(g) {
        double t = y[0] * at(v[0], *g, kk, i, j);
        for (int q = 1; q < k; q++) { const double p = y[q] * at(v[q], *g, kk, i, j); t = t + p; }
        at(out, *g, kk, i, j) = t;
    }
    return 0;
}
int mgk_scale_to_f64(mgk_ctx *c, const mgk_geom *g, double a, const double *x, double *out, double *out2, void *) {
    if (!c || c->capturing || !g || !x || !out || out == out2) return fail(MGK_EINVAL, "mgk_scale_to_f64");
    g_kry_calls[4]++;
    KRY_INTERIOR(g) {
        const double t = a * at(x, *g, kk, i, j);
        at(out, *g, kk, i, j) = t;
        if (out2) at(out2, *g, kk, i, j) = t;
    }
    return 0;
}
}   // extern "C"
