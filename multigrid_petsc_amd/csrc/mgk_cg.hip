// mgk_cg.hip -- the two fused passes of V-cycle-preconditioned conjugate gradients (csrc/mg_cg.c, include/mgk_cg.h) on
// level fields, each reading its operands ONCE:
//   mgk_cg_direction_apply_dot_f64  p_new = z + beta p_old, q = A p_new, sigma = p_new . q       32 B per unknown (first step, p_new = z: 24 B)
//   mgk_cg_update_sumsq_f64         x += alpha p, r -= alpha q, sum r^2 of the new r              48 B per unknown
// Written with mgk_flat_aypx + mgk_apply_f64 + mgk_flat_dot and two mgk_flat_axpy + mgk_sumsq_f64 a step moves 56 + 56 B in six launches.  A CG
// step is then: one cycle, the 16 B dot r . z (mgk_multi_dot_f64, k = 1), the 32 B direction pass, the 48 B update pass -- 96 B per fine
// unknown beside the cycle, three host synchronisations (rho', sigma, r . r).
// fp64, padded level layout, 2-D and 3-D, constant coefficients, no FMA (-ffp-contract=off), A in the canonical order;
// only interior points are summed and stored.  Reductions: one partial per block in the CALLER's workspace (mgk_cg_ws: the context's shared
// scratch is not touched), finished in a fixed order by one block -- no floating-point atomics, the same bits on every run.
// Direction pass: independent waves, a lane owns a column pair, the x neighbours come by DPP shifts and the two wave-edge lanes load theirs.
// A wave marches along the last axis (2-D: y, 3-D: z over a strip of TY rows plus one halo row a side) with the planes m-1, m, m+1 of p_new
// in registers; the halo values of p_new are recomputed from z and p_old (their ghost ring is 0, so 0 + beta 0 = 0 there: the Dirichlet
// convention), and the loads of plane m+2 are issued before plane m is used.  p_new is another buffer than p_old: neighbouring tiles read the
// old halo values while this one stores.  The dot takes a wave's own points only.
// Stores: by field size, as in mgk_krylov.hip; mgk_set_tuning(variant = 0 / 1) forces one policy.
// The workspace, the direction kernel (one template with the fp32-z form of mgk_cg_mixed.hip) and the fixed-order finish: mgk_cg_dev.hpp.
#include "mgk_cg_dev.hpp"
#include <new>

namespace {

struct CgUpdArgs {
    int nx, ny, npairs, nt;
    long pitch, plane, nrows;       // nrows = ny * nz
    double alpha;
};

// the row walk of k_multi_axpy_sumsq (mgk_krylov.hip): a lane owns a column pair and walks down its block's share of the rows
__global__ void __launch_bounds__(256) k_cg_update(const CgUpdArgs a, const double *__restrict__ p, const double *__restrict__ q,
                                                   double *__restrict__ x, double *__restrict__ r, double *__restrict__ parts) {
    __shared__ double red[16];
    const int pr = blockIdx.x * blockDim.x + threadIdx.x;
    const int x0 = 2 * pr;
    const bool half = x0 + 1 == a.nx;
    const bool nt = a.nt < 0 ? mgk_store_nt_2d((int)(a.nrows > 0x7fffffffL ? 0x7fffffffL : a.nrows), a.pitch) : a.nt != 0;
    double acc = 0.0;
    if (pr < a.npairs) {
        const long rpb = (a.nrows + gridDim.y - 1) / gridDim.y;
        const long row0 = (long)blockIdx.y * rpb, row1 = row0 + rpb < a.nrows ? row0 + rpb : a.nrows;
        for (long row = row0; row < row1; row++) {
            const long k = row / a.ny, i = row - k * a.ny;
            const long o = k * a.plane + i * a.pitch + x0;
            const double2 pv = ld2(p + o, true), qv = ld2(q + o, true);
            double2 xv = ld2(x + o, true), rv = ld2(r + o, true);
            const double px = a.alpha * pv.x, py = a.alpha * pv.y, qx = a.alpha * qv.x, qy = a.alpha * qv.y;
            xv.x = xv.x + px; xv.y = xv.y + py;
            rv.x = rv.x - qx; rv.y = rv.y - qy;
            cg_store(x + o, xv, half, nt);
            cg_store(r + o, rv, half, nt);
            const double sx = rv.x * rv.x, sy = half ? 0.0 : rv.y * rv.y;
            acc += sx + sy;
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) parts[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

}  // namespace

MGK_PRELOAD_UNIT(k_cg_finish)

extern "C" int mgk_cg_workspace_create(mgk_ctx *c, mgk_cg_ws **out) {
    if (!c || !out) return fail(MGK_EINVAL, "mgk_cg_workspace_create: bad arguments");
    *out = nullptr;
    mgk_cg_ws *ws = new (std::nothrow) mgk_cg_ws();
    if (!ws) return fail(MGK_EINVAL, "mgk_cg_workspace_create: out of host memory");
    ws->slots = ws->res_dev = ws->land = nullptr;
    ws->nslots = CG_SLOTS;
    void *p = nullptr;
    int rc = mgk_malloc(c, &p, sizeof(double) * CG_SLOTS);
    ws->slots = (double *)p; p = nullptr;
    if (!rc) { rc = mgk_malloc(c, &p, sizeof(double) * 2); ws->res_dev = (double *)p; p = nullptr; }
    if (!rc) { rc = mgk_host_alloc(c, &p, sizeof(double) * 2); ws->land = (double *)p; }
    if (rc) { mgk_cg_workspace_destroy(c, ws); return rc; }
    *out = ws;
    return 0;
}

extern "C" void mgk_cg_workspace_destroy(mgk_ctx *c, mgk_cg_ws *ws) {
    if (!c || !ws) return;
    if (ws->slots) mgk_free(c, ws->slots);
    if (ws->res_dev) mgk_free(c, ws->res_dev);
    if (ws->land) mgk_host_free(c, ws->land);
    delete ws;
}

extern "C" int mgk_cg_workspace_debug(mgk_cg_ws *ws, double **parts_dev, int *nslots) {
    if (!ws || !parts_dev || !nslots) return fail(MGK_EINVAL, "mgk_cg_workspace_debug: bad arguments");
    *parts_dev = ws->slots;
    *nslots = ws->nslots;
    return 0;
}

extern "C" int mgk_cg_direction_apply_dot_f64(mgk_ctx *c, const mgk_geom *g, const double *coef, double beta, const double *z, const double *p_old,
                                              double *p_new, double *q, mgk_cg_ws *ws, double *sigma_host, void *stream) {
    if (!c || !coef || !z || !p_new || !q || !ws) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: null argument");
    if (!cg_geom_ok(g)) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: not a level geometry (2-D or 3-D, odd nx)");
    if (p_new == p_old || p_new == z || q == z || q == p_old || q == p_new)
        return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: p_new must differ from p_old and z, q from z, p_old and p_new");
    if (p_old && !std::isfinite(beta)) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: beta is not finite");
    hipStream_t s = S(c, stream);
    bool busy = false;
    if (int rc = cg_capturing(s, &busy)) return rc;
    if (busy) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: the stream is being captured (the sum is copied to the host)");
    CgDirArgs a;
    const long nblk = cg_direction_shape(g, coef, beta, !p_old, ws, a);
    if (nblk < 1) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: more blocks than workspace slots");
    const double *zz = z + g->org, *po = p_old ? p_old + g->org : nullptr;
    double *pn = p_new + g->org, *qq = q + g->org;
#define CG_LAUNCH(DIM, TY, FIRST) hipLaunchKernelGGL((k_cg_direction<DIM, TY, FIRST, double>), dim3((unsigned)nblk), dim3(256), 0, s, a, zz, po, pn, qq, ws->slots)
    if (g->dim == 3) { if (p_old) CG_LAUNCH(3, CG_TY, false); else CG_LAUNCH(3, CG_TY, true); }
    else { if (p_old) CG_LAUNCH(2, 1, false); else CG_LAUNCH(2, 1, true); }
#undef CG_LAUNCH
    HIPCHK(hipGetLastError());
    return cg_finish(ws, (int)nblk, 0, s, sigma_host);
}

extern "C" int mgk_cg_update_sumsq_f64(mgk_ctx *c, const mgk_geom *g, double alpha, const double *p, const double *q, double *x, double *r,
                                       mgk_cg_ws *ws, double *sumsq_host, void *stream) {
    if (!c || !p || !q || !x || !r || !ws) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64: null argument");
    if (!cg_geom_ok(g)) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64: not a level geometry (2-D or 3-D, odd nx)");
    if (p == q || p == x || p == r || q == x || q == r || x == r) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64: p, q, x and r must be four different fields");
    hipStream_t s = S(c, stream);
    bool busy = false;
    if (int rc = cg_capturing(s, &busy)) return rc;
    if (busy) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64: the stream is being captured (the sum is copied to the host)");
    CgUpdArgs a;
    memset(&a, 0, sizeof(a));
    a.nx = g->nx; a.ny = g->ny; a.npairs = (g->nx + 1) / 2; a.nt = store_policy();
    a.pitch = g->pitch; a.plane = g->plane; a.nrows = (long)g->ny * g->nz;
    a.alpha = alpha;
    const unsigned gx = (a.npairs + 255) / 256;
    long gy = a.nrows, cap = (ws->nslots < 2048 ? ws->nslots : 2048) / (long)gx;
    if (cap < 1) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64: more blocks than workspace slots");
    if (gy > cap) gy = cap;
    hipLaunchKernelGGL(k_cg_update, dim3(gx, (unsigned)gy), dim3(256), 0, s, a, p + g->org, q + g->org, x + g->org, r + g->org, ws->slots);
    HIPCHK(hipGetLastError());
    return cg_finish(ws, (int)(gx * gy), 1, s, sumsq_host);
}
