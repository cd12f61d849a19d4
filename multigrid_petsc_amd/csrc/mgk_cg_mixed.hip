// mgk_cg_mixed.hip -- the three passes that join the fp64 recurrence of conjugate gradients to the fp32 V-cycle of the mixed-precision solver
// (csrc/mg_cg_mixed.c, include/mgk_cg_mixed.h), each reading its operands ONCE:
//   mgk_cg_dot_f64_f32                   sum r * (double) z32                                                       12 B per unknown
//   mgk_cg_direction_apply_dot_zf32_f64  p_new = (double) z32 + beta p_old, q = A p_new, sigma = p_new . q          28 B (first step: 20 B)
//   mgk_cg_update_sumsq_f64_f32          x += alpha p, r -= alpha q, sum r^2, r32 = (float) r [, e0 = scale32 * (r32 * dinv32)]   52 B (56 B)
// Built from the parent's kernels a step needs mgk_correct_f64_from_f32 into a zeroed field (12 B, after an 8 B memset) before the fp64 dot and
// direction passes, and mgk_residual_f64_to_f32_jz (28 B, a stencil) after the fp64 update pass: 144 B and more against 92-96 B here.
// 3-D only; fp64 fields in the layout of g, fp32 fields in that of g32; no FMA (-ffp-contract=off), A in the canonical order; (double) of a float
// is exact, (float) of a double rounds to nearest.  Only interior points are summed and stored.  Reductions as in mgk_cg.hip: one partial per
// block in the CALLER's workspace, finished in a fixed order by one block.
// The direction pass is k_cg_direction of mgk_cg_dev.hpp with ZT = float: the same march, the planes of z32 in flight as float pairs (12 VGPRs
// where the fp64 form holds 24), converted where p_new is formed.  The dot and the update are row walks like k_cg_update: a lane owns a column
// pair, 16 B of every fp64 field and 8 B of every fp32 one.
#include "mgk_cg_dev.hpp"
#include "mgk_cg_mixed.h"

namespace {

struct CgMixArgs {
    int nx, ny, npairs, nt;
    long pitch, plane, pitch32, plane32, nrows;     // nrows = ny * nz
    double alpha;
    float dinv32, scale32;
};

typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void cg_store32(float *p, float2 v, bool half, bool nt) {
    if (half) { *p = v.x; return; }
    if (nt) { f2v t; t.x = v.x; t.y = v.y; __builtin_nontemporal_store(t, reinterpret_cast<f2v *>(p)); }
    else *reinterpret_cast<float2 *>(p) = v;
}

__global__ void __launch_bounds__(256) k_cg_dot_f32(const CgMixArgs a, const double *__restrict__ r, const float *__restrict__ z, double *__restrict__ parts) {
    __shared__ double red[16];
    const int pr = blockIdx.x * blockDim.x + threadIdx.x;
    const int x0 = 2 * pr;
    const bool half = x0 + 1 == a.nx;
    double acc = 0.0;
    if (pr < a.npairs) {
        const long rpb = (a.nrows + gridDim.y - 1) / gridDim.y;
        const long row0 = (long)blockIdx.y * rpb, row1 = row0 + rpb < a.nrows ? row0 + rpb : a.nrows;
        for (long row = row0; row < row1; row++) {
            const long k = row / a.ny, i = row - k * a.ny;
            const double2 rv = ld2(r + k * a.plane + i * a.pitch + x0, true);
            const float2 zv = cg_ldz2(z + k * a.plane32 + i * a.pitch32 + x0, true);
            const double px = rv.x * (double)zv.x, py = half ? 0.0 : rv.y * (double)zv.y;
            acc += px + py;
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) parts[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// JZ: also e0 = scale32 * (r32 * dinv32), k_jacobi_zero<float>'s arithmetic on the value just stored
template <bool JZ>
__global__ void __launch_bounds__(256) k_cg_update_f32(const CgMixArgs a, const double *__restrict__ p, const double *__restrict__ q, double *__restrict__ x,
                                                       double *__restrict__ r, float *__restrict__ r32, float *__restrict__ e0, double *__restrict__ parts) {
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
            const long o = k * a.plane + i * a.pitch + x0, o32 = k * a.plane32 + i * a.pitch32 + x0;
            const double2 pv = ld2(p + o, true), qv = ld2(q + o, true);
            double2 xv = ld2(x + o, true), rv = ld2(r + o, true);
            const double px = a.alpha * pv.x, py = a.alpha * pv.y, qx = a.alpha * qv.x, qy = a.alpha * qv.y;
            xv.x = xv.x + px; xv.y = xv.y + py;
            rv.x = rv.x - qx; rv.y = rv.y - qy;
            cg_store(x + o, xv, half, nt);
            cg_store(r + o, rv, half, nt);
            float2 rf;
            rf.x = (float)rv.x; rf.y = (float)rv.y;
            cg_store32(r32 + o32, rf, half, nt);
            if (JZ) {
                const float zx = rf.x * a.dinv32, zy = rf.y * a.dinv32;
                float2 ef;
                ef.x = a.scale32 * zx; ef.y = a.scale32 * zy;
                cg_store32(e0 + o32, ef, half, nt);
            }
            const double sx = rv.x * rv.x, sy = half ? 0.0 : rv.y * rv.y;
            acc += sx + sy;
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) parts[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

bool cg_mixed_geoms_ok(const mgk_geom *g, const mgk_geom *g32) {
    return cg_geom_ok(g) && g->dim == 3 && g32 && g32->dim == 3 && g32->nx == g->nx && g32->ny == g->ny && g32->nz == g->nz &&
           g32->pitch >= 32 + g->nx + 1 && g32->plane >= g32->pitch * (g->ny + 2);
}
// the grid of the two row walks: blocks of 256 column pairs across, the rows shared among gy blocks; gy = 0: more blocks than slots
void cg_mixed_rows(const mgk_geom *g, const mgk_geom *g32, const mgk_cg_ws *ws, CgMixArgs &a, unsigned *gx, long *gy) {
    memset(&a, 0, sizeof(a));
    a.nx = g->nx; a.ny = g->ny; a.npairs = (g->nx + 1) / 2; a.nt = store_policy();
    a.pitch = g->pitch; a.plane = g->plane; a.pitch32 = g32->pitch; a.plane32 = g32->plane; a.nrows = (long)g->ny * g->nz;
    *gx = (a.npairs + 255) / 256;
    const long cap = (ws->nslots < 2048 ? ws->nslots : 2048) / (long)*gx;
    *gy = a.nrows < cap ? a.nrows : cap;
}

}  // namespace

MGK_PRELOAD_UNIT(k_cg_dot_f32)

extern "C" int mgk_cg_dot_f64_f32(mgk_ctx *c, const mgk_geom *g, const mgk_geom *g32, const double *r, const float *z32, mgk_cg_ws *ws,
                                  double *dot_host, void *stream) {
    if (!c || !r || !z32 || !ws) return fail(MGK_EINVAL, "mgk_cg_dot_f64_f32: null argument");
    if (!cg_mixed_geoms_ok(g, g32)) return fail(MGK_EINVAL, "mgk_cg_dot_f64_f32: not a 3-D level geometry and its fp32 twin (odd nx, equal extents)");
    if ((const void *)r == (const void *)z32) return fail(MGK_EINVAL, "mgk_cg_dot_f64_f32: r and z32 must be two different fields");
    hipStream_t s = S(c, stream);
    bool busy = false;
    if (int rc = cg_capturing(s, &busy)) return rc;
    if (busy) return fail(MGK_EINVAL, "mgk_cg_dot_f64_f32: the stream is being captured (the sum is copied to the host)");
    CgMixArgs a;
    unsigned gx;
    long gy;
    cg_mixed_rows(g, g32, ws, a, &gx, &gy);
    if (gy < 1) return fail(MGK_EINVAL, "mgk_cg_dot_f64_f32: more blocks than workspace slots");
    hipLaunchKernelGGL(k_cg_dot_f32, dim3(gx, (unsigned)gy), dim3(256), 0, s, a, r + g->org, z32 + g32->org, ws->slots);
    HIPCHK(hipGetLastError());
    return cg_finish(ws, (int)(gx * gy), 0, s, dot_host);
}

extern "C" int mgk_cg_direction_apply_dot_zf32_f64(mgk_ctx *c, const mgk_geom *g, const mgk_geom *g32, const double *coef, double beta, const float *z32,
                                                   const double *p_old, double *p_new, double *q, mgk_cg_ws *ws, double *sigma_host, void *stream) {
    if (!c || !coef || !z32 || !p_new || !q || !ws) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: null argument");
    if (!cg_mixed_geoms_ok(g, g32))
        return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: not a 3-D level geometry and its fp32 twin (odd nx, equal extents)");
    const void *zv = z32;
    if (p_new == p_old || q == p_old || q == p_new || zv == p_new || zv == q || zv == p_old)
        return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: p_new must differ from p_old, q from p_old and p_new, and none may be z32");
    if (p_old && !std::isfinite(beta)) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: beta is not finite");
    hipStream_t s = S(c, stream);
    bool busy = false;
    if (int rc = cg_capturing(s, &busy)) return rc;
    if (busy) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: the stream is being captured (the sum is copied to the host)");
    CgDirArgs a;
    const long nblk = cg_direction_shape(g, coef, beta, !p_old, ws, a);
    if (nblk < 1) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_zf32_f64: more blocks than workspace slots");
    a.zpitch = g32->pitch; a.zms = g32->plane;
    const float *zz = z32 + g32->org;
    const double *po = p_old ? p_old + g->org : nullptr;
    double *pn = p_new + g->org, *qq = q + g->org;
    if (p_old) hipLaunchKernelGGL((k_cg_direction<3, CG_TY, false, float>), dim3((unsigned)nblk), dim3(256), 0, s, a, zz, po, pn, qq, ws->slots);
    else hipLaunchKernelGGL((k_cg_direction<3, CG_TY, true, float>), dim3((unsigned)nblk), dim3(256), 0, s, a, zz, po, pn, qq, ws->slots);
    HIPCHK(hipGetLastError());
    return cg_finish(ws, (int)nblk, 0, s, sigma_host);
}

extern "C" int mgk_cg_update_sumsq_f64_f32(mgk_ctx *c, const mgk_geom *g, const mgk_geom *g32, double alpha, const double *p, const double *q, double *x,
                                           double *r, float *r32, float *e0, double dinv, double scale, mgk_cg_ws *ws, double *sumsq_host, void *stream) {
    if (!c || !p || !q || !x || !r || !r32 || !ws) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64_f32: null argument");
    if (!cg_mixed_geoms_ok(g, g32)) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64_f32: not a 3-D level geometry and its fp32 twin (odd nx, equal extents)");
    const void *f[6] = {p, q, x, r, r32, e0};
    for (int i = 0; i < 6; i++)
        for (int j = i + 1; j < 6; j++)
            if (f[i] && f[i] == f[j]) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64_f32: p, q, x, r, r32 and e0 must be different fields");
    hipStream_t s = S(c, stream);
    bool busy = false;
    if (int rc = cg_capturing(s, &busy)) return rc;
    if (busy) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64_f32: the stream is being captured (the sum is copied to the host)");
    CgMixArgs a;
    unsigned gx;
    long gy;
    cg_mixed_rows(g, g32, ws, a, &gx, &gy);
    if (gy < 1) return fail(MGK_EINVAL, "mgk_cg_update_sumsq_f64_f32: more blocks than workspace slots");
    a.alpha = alpha; a.dinv32 = (float)dinv; a.scale32 = (float)scale;
    float *e = e0 ? e0 + g32->org : nullptr;
    if (e0) hipLaunchKernelGGL(k_cg_update_f32<true>, dim3(gx, (unsigned)gy), dim3(256), 0, s, a, p + g->org, q + g->org, x + g->org, r + g->org, r32 + g32->org, e, ws->slots);
    else hipLaunchKernelGGL(k_cg_update_f32<false>, dim3(gx, (unsigned)gy), dim3(256), 0, s, a, p + g->org, q + g->org, x + g->org, r + g->org, r32 + g32->org, e, ws->slots);
    HIPCHK(hipGetLastError());
    return cg_finish(ws, (int)(gx * gy), 1, s, sumsq_host);
}
