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
#include "mgk_dev.hpp"
#include "mgk_cg.h"
#include <new>

struct mgk_cg_ws {
    double *slots;          // CG_SLOTS per-block partial sums (device)
    double *res_dev;        // 2 reduced values (device): sigma, sum r^2
    double *land;           // their pinned landing area (host)
    int nslots;
};

namespace {

const int CG_SLOTS = 8192;
const int CG_TY = 4;        // rows of a 3-D strip: 3 planes x (TY + 2) rows of p_new and the loads in flight are 218 VGPRs (first step: 152), no scratch, two waves per SIMD

struct CgDirArgs {
    int nx, ny, npairs, wavesx, nstrips, M, mlen;       // M: extent of the marching axis, cut into chunks of mlen
    long pitch, ms, nwaves;                             // ms: stride of the marching axis
    int nt;
    double a0, a1, a2, a3, a4, a5, a6, beta;            // {m-1, i-1, j-1, C, j+1, i+1, m+1}; 2-D: a1 = a5 = 0 and the marching axis is y
};

__device__ __forceinline__ void cg_store(double *p, double2 v, bool half, bool nt) {
    if (half) { *p = v.x; return; }
    V16<double> t; t.v[0] = v.x; t.v[1] = v.y;
    stv_policy(p, t, nt);
}

// DIM 2: one row per marching step (TY = 1, no halo rows); DIM 3: TY rows and one halo row a side.  FIRST: p_new = z, p_old is not read
template <int DIM, int TY, bool FIRST>
__global__ void __launch_bounds__(256) k_cg_direction(const CgDirArgs a, const double *__restrict__ z, const double *__restrict__ po,
                                                      double *__restrict__ pn, double *__restrict__ q, double *__restrict__ parts) {
    constexpr int H = DIM == 3 ? 1 : 0, NR = TY + 2 * H;
    __shared__ double red[16];
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    double acc = 0.0;
    if (w < a.nwaves) {                                              // uniform over the wave: the DPP shifts below run with every lane enabled
        const int wx = (int)(w % a.wavesx);
        const long t_ = w / a.wavesx;
        const int st = (int)(t_ % a.nstrips), ch = (int)(t_ / a.nstrips);
        const int x0 = 2 * (wx * 64 + lane);
        const bool on = wx * 64 + lane < a.npairs, half = x0 + 1 == a.nx;
        const bool nt = a.nt < 0 ? mgk_store_nt_2d(DIM == 3 ? a.M * (a.ny + 2) : a.ny, a.pitch) : a.nt != 0;
        const int i0 = DIM == 3 ? st * TY : 0;
        const int m0 = ch * a.mlen, m1 = m0 + a.mlen < a.M ? m0 + a.mlen : a.M;
        long roff[NR];
        bool rd[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) {
            roff[r] = (DIM == 3 ? (long)(i0 - H + r) * a.pitch : 0) + x0;
            rd[r] = on && (DIM == 2 || i0 - H + r <= a.ny);
        }
        // the wave-edge lanes' x neighbour: lane 0 column x0 - 1, lane 63 column x0 + 2 (both within the row: ghost column or interior)
        const bool edge = on && (lane == 0 || (lane == 63 && x0 + 2 <= a.nx));
        const int eoff = lane == 0 ? -1 : 2;
        double2 A[NR], B[NR], Cn[NR], zr[NR], pr[NR];
#define CG_LOAD(m)                                                                                   \
        _Pragma("unroll") for (int r = 0; r < NR; r++) {                                             \
            const long o_ = (long)(m) * a.ms + roff[r];                                              \
            zr[r] = ld2(z + o_, rd[r]);                                                              \
            if (!FIRST) pr[r] = ld2(po + o_, rd[r]);                                                 \
        }
#define CG_COMBINE(dst)                                                                              \
        _Pragma("unroll") for (int r = 0; r < NR; r++) {                                             \
            if (FIRST) dst[r] = zr[r];                                                               \
            else { const double tx_ = a.beta * pr[r].x, ty_ = a.beta * pr[r].y; dst[r].x = zr[r].x + tx_; dst[r].y = zr[r].y + ty_; } \
        }
        CG_LOAD(m0 - 1) CG_COMBINE(A)
        CG_LOAD(m0) CG_COMBINE(B)
        CG_LOAD(m0 + 1)
        for (int m = m0; m < m1; m++) {
            double e[TY];
#pragma unroll
            for (int r = 0; r < TY; r++) {
                const long o_ = (long)m * a.ms + roff[r + H] + eoff;
                const bool ok = edge && (DIM == 2 || i0 + r < a.ny);
                const double ze = ld1(z + o_, ok);
                if (FIRST) e[r] = ze;
                else { const double t_ = a.beta * ld1(po + o_, ok); e[r] = ze + t_; }
            }
            CG_COMBINE(Cn)
            if (m + 1 < m1) { CG_LOAD(m + 2) }
#pragma unroll
            for (int r = 0; r < TY; r++) {
                const int c = r + H;
                const double W = lane_up_old(B[c].y, e[r]), E = lane_dn_old(B[c].x, e[r]);
                double2 t;
                t.x = a.a0 * A[c].x;                       t.y = a.a0 * A[c].y;
                if (DIM == 3) { t.x = t.x + a.a1 * B[c - H].x; t.y = t.y + a.a1 * B[c - H].y; }
                t.x = t.x + a.a2 * W;                      t.y = t.y + a.a2 * B[c].x;
                t.x = t.x + a.a3 * B[c].x;                 t.y = t.y + a.a3 * B[c].y;
                t.x = t.x + a.a4 * B[c].y;                 t.y = t.y + a.a4 * E;
                if (DIM == 3) { t.x = t.x + a.a5 * B[c + H].x; t.y = t.y + a.a5 * B[c + H].y; }
                t.x = t.x + a.a6 * Cn[c].x;                t.y = t.y + a.a6 * Cn[c].y;
                if (on && (DIM == 2 || i0 + r < a.ny)) {
                    const long o_ = (long)m * a.ms + roff[c];
                    cg_store(pn + o_, B[c], half, nt);
                    cg_store(q + o_, t, half, nt);
                    const double px = B[c].x * t.x, py = half ? 0.0 : B[c].y * t.y;
                    acc += px + py;
                }
            }
#pragma unroll
            for (int r = 0; r < NR; r++) { A[r] = B[r]; B[r] = Cn[r]; }
        }
#undef CG_LOAD
#undef CG_COMBINE
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

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

// out[0] = the n partial sums added up in a fixed order
__global__ void __launch_bounds__(256) k_cg_finish(const double *__restrict__ parts, int n, double *__restrict__ out) {
    __shared__ double red[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += parts[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

bool cg_geom_ok(const mgk_geom *g) {
    return g && (g->dim == 2 || g->dim == 3) && g->nx >= 1 && g->ny >= 1 && g->nz >= 1 && (g->nx & 1) && (g->dim == 3 || g->nz == 1);
}
int cg_capturing(hipStream_t s, bool *busy) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &st));
    *busy = st != hipStreamCaptureStatusNone;
    return 0;
}
// the partials [0, nblk) of the workspace -> result slot `slot`, its landing area, and the host if asked
int cg_finish(mgk_cg_ws *ws, int nblk, int slot, hipStream_t s, double *host) {
    hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(256), 0, s, ws->slots, nblk, ws->res_dev + slot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ws->land + slot, ws->res_dev + slot, sizeof(double), hipMemcpyDeviceToHost, s));
    if (host) {
        HIPCHK(hipStreamSynchronize(s));
        *host = ws->land[slot];
    }
    return 0;
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
    memset(&a, 0, sizeof(a));
    const int ty = g->dim == 3 ? CG_TY : 1;
    a.nx = g->nx; a.ny = g->ny; a.npairs = (g->nx + 1) / 2; a.wavesx = (a.npairs + 63) / 64;
    a.nstrips = g->dim == 3 ? (g->ny + ty - 1) / ty : 1;
    a.M = g->dim == 3 ? g->nz : g->ny;
    a.pitch = g->pitch; a.ms = g->dim == 3 ? g->plane : g->pitch;
    a.nt = store_policy();
    a.beta = p_old ? beta : 0.0;
    if (g->dim == 3) set_coef7(a, coef); else set_coef5(a, coef);
    // chunks of the marching axis: enough waves to fill the chip, chunks of 32 planes or more (every chunk re-reads two halo planes),
    // never more blocks than the workspace has slots
    const long tiles = (long)a.wavesx * a.nstrips, target = 16384;
    long nch = tiles >= target ? 1 : (target + tiles - 1) / tiles;
    if (nch > (a.M + 31) / 32) nch = (a.M + 31) / 32;
    if (g_zchunk > 0) nch = (a.M + g_zchunk - 1) / g_zchunk;
    const long cap = 4L * ws->nslots / tiles;
    if (nch > cap) nch = cap;
    if (nch < 1) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: more blocks than workspace slots");
    a.mlen = (int)((a.M + nch - 1) / nch);
    nch = (a.M + a.mlen - 1) / a.mlen;
    a.nwaves = tiles * nch;
    const long nblk = (a.nwaves + 3) / 4;
    if (nblk > ws->nslots) return fail(MGK_EINVAL, "mgk_cg_direction_apply_dot_f64: more blocks than workspace slots");
    const double *zz = z + g->org, *po = p_old ? p_old + g->org : nullptr;
    double *pn = p_new + g->org, *qq = q + g->org;
#define CG_LAUNCH(DIM, TY, FIRST) hipLaunchKernelGGL((k_cg_direction<DIM, TY, FIRST>), dim3((unsigned)nblk), dim3(256), 0, s, a, zz, po, pn, qq, ws->slots)
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
