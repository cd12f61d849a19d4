// mock_mgk_cg_mixed.cpp -- host-memory stand-ins for the entry points of include/mgk_cg_mixed.h (mgk_cg_dot_f64_f32,
// mgk_cg_direction_apply_dot_zf32_f64, mgk_cg_update_sumsq_f64_f32) in the stated arithmetic: interior points only, (double) of a float exact,
// p_new = (double) z32 + (beta * p_old), A in the canonical order with every product and sum rounded separately, x + (alpha * p),
// r - (alpha * q), r32 = (float) r, e0 = (float) scale * (r32 * (float) dinv) in fp32; the sums in long double like the other reductions of
// mock_mgk.cpp.  tests/mock_mgk_cg.cpp (the fp64 passes, the workspace, the allocation that can be told to fail, and through it the GMRES and the
// plain stand-ins) is included textually and stays as it is.  Linked with mg_solver.c, mg_comm.c, mg_cg.c, mg_cg_mixed.c and mg_gmres.c by
// tests/test_cg_mixed_cpu.py.  The three passes count their calls: mock_cg_mixed_calls(0 / 1 / 2) = dot / direction / update.
#include "mock_mgk_cg.cpp"
#include "mgk_cg_mixed.h"

static int g_cgm_calls[3] = {0, 0, 0};
extern "C" int mock_cg_mixed_calls(int which) { return (which >= 0 && which < 3) ? g_cgm_calls[which] : -1; }
extern "C" void mock_cg_mixed_calls_reset(void) { g_cgm_calls[0] = g_cgm_calls[1] = g_cgm_calls[2] = 0; mock_cg_calls_reset(); }

static bool cgm_geoms(const mgk_geom *g, const mgk_geom *h) {
    return g && h && g->dim == 3 && h->dim == 3 && (g->nx & 1) && g->nx == h->nx && g->ny == h->ny && g->nz == h->nz;
}

extern "C" {
int mgk_cg_dot_f64_f32(mgk_ctx *c, const mgk_geom *g, const mgk_geom *g32, const double *r, const float *z32, mgk_cg_ws *ws, double *dot_host, void *) {
    if (!c || !r || !z32 || !ws) return fail(MGK_EINVAL, "mgk_cg_dot_f64_f32: null argument");
    if (!cgm_geoms(g, g32)) return fail(MGK_EINVAL, "mgk_cg_dot_f64_f32: not a 3-D level geometry and its fp32 twin");
    if (c->capturing) return fail(MGK_EINVAL, "mgk_cg_dot_f64_f32: the stream is being captured");
    if ((const void *)r == (const void *)z32) return fail(MGK_EINVAL, "mgk_cg_dot_f64_f32: aliasing");
    g_cgm_calls[0]++;
    long double s = 0;
    KRY_INTERIOR(g) s += (long double)(at(r, *g, kk, i, j) * (double)at(z32, *g32, kk, i, j));
    ws->slots[0] = (double)s;
    if (dot_host) *dot_host = (double)s;
    return 0;
}

int mgk_cg_direction_apply_dot_zf32_f64(mgk_ctx *c, const mgk_geom *g, const mgk_geom *g32, const double *coef, double beta, const float *z32,
                                        const double *p_old, double *p_new, double *q, mgk_cg_ws *ws, double *sigma_host, void *) {
    if (!c || !coef || !z32 || !p_new || !q || !ws) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: null argument");
    if (!cgm_geoms(g, g32)) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: not a 3-D level geometry and its fp32 twin");
    if (c->capturing) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: the stream is being captured");
    const void *zv = z32;
    if (p_new == p_old || q == p_old || q == p_new || zv == p_new || zv == q || zv == p_old) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: aliasing");
    g_cgm_calls[1]++;
    KRY_INTERIOR(g) {
        double v = (double)at(z32, *g32, kk, i, j);
        if (p_old) { const double t = beta * at(p_old, *g, kk, i, j); v = v + t; }
        at(p_new, *g, kk, i, j) = v;
    }
    long double s = 0;
    KRY_INTERIOR(g) {                                                   // (the ghost ring of p_new is zero: the driver's fields come zero-filled)
        double t = coef[0] * at(p_new, *g, kk - 1, i, j);
        t = t + coef[1] * at(p_new, *g, kk, i - 1, j);
        t = t + coef[2] * at(p_new, *g, kk, i, j - 1);
        t = t + coef[3] * at(p_new, *g, kk, i, j);
        t = t + coef[4] * at(p_new, *g, kk, i, j + 1);
        t = t + coef[5] * at(p_new, *g, kk, i + 1, j);
        t = t + coef[6] * at(p_new, *g, kk + 1, i, j);
        at(q, *g, kk, i, j) = t;
        s += (long double)(at(p_new, *g, kk, i, j) * t);
    }
    ws->slots[0] = (double)s;
    if (sigma_host) *sigma_host = (double)s;
    return 0;
}

int mgk_cg_update_sumsq_f64_f32(mgk_ctx *c, const mgk_geom *g, const mgk_geom *g32, double alpha, const double *p, const double *q, double *x, double *r,
                                float *r32, float *e0, double dinv, double scale, mgk_cg_ws *ws, double *sumsq_host, void *) {
    if (!c || !p || !q || !x || !r || !r32 || !ws) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64_f32: null argument");
    if (!cgm_geoms(g, g32)) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64_f32: not a 3-D level geometry and its fp32 twin");
    if (c->capturing) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64_f32: the stream is being captured");
    const void *f[6] = {p, q, x, r, r32, e0};
    for (int a = 0; a < 6; a++) for (int b = a + 1; b < 6; b++) if (f[a] && f[a] == f[b]) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64_f32: aliasing");
    g_cgm_calls[2]++;
    const float d32 = (float)dinv, s32 = (float)scale;
    long double s = 0;
    KRY_INTERIOR(g) {
        const double tp = alpha * at(p, *g, kk, i, j), tq = alpha * at(q, *g, kk, i, j);
        at(x, *g, kk, i, j) = at(x, *g, kk, i, j) + tp;
        const double rr = at(r, *g, kk, i, j) - tq;
        at(r, *g, kk, i, j) = rr;
        const float rf = (float)rr;
        at(r32, *g32, kk, i, j) = rf;
        if (e0) { const float zx = rf * d32; at(e0, *g32, kk, i, j) = s32 * zx; }
        s += (long double)(rr * rr);
    }
    ws->slots[1] = (double)s;
    if (sumsq_host) *sumsq_host = (double)s;
    return 0;
}
}   // extern "C"
