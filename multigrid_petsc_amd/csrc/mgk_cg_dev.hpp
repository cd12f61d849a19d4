// mgk_cg_dev.hpp -- what the two units of the CG passes share (mgk_cg.hip: fp64, include/mgk_cg.h; mgk_cg_mixed.hip: the fp64 recurrence over an
// fp32 preconditioner, include/mgk_cg_mixed.h): the reduction workspace, its fixed-order finish, the checks of the launchers, and the direction
// kernel, which is ONE template for both -- ZT is the type z is read in (double: DESIGN.md section 8l; float: section 8m, converted exactly on the
// way in).  Everything sits in an unnamed namespace: each unit has its own copy of the kernels it instantiates.
#pragma once
#include "mgk_dev.hpp"
#include "mgk_cg.h"

struct mgk_cg_ws {
    double *slots;          // CG_SLOTS per-block partial sums (device)
    double *res_dev;        // 2 reduced values (device): sigma / r . z, sum r^2
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
    long zpitch, zms;                                   // z in fp32: its own row and plane strides (an fp64 z has those of the other fields: not read)
};

__device__ __forceinline__ void cg_store(double *p, double2 v, bool half, bool nt) {
    if (half) { *p = v.x; return; }
    V16<double> t; t.v[0] = v.x; t.v[1] = v.y;
    stv_policy(p, t, nt);
}

// a column pair / one value of z in the type it is stored in; (double) of a float is exact
template <typename ZT> struct CgPair;
template <> struct CgPair<double> { typedef double2 type; };
template <> struct CgPair<float> { typedef float2 type; };
__device__ __forceinline__ double2 cg_ldz2(const double *p, bool ok) { return ld2(p, ok); }
__device__ __forceinline__ float2 cg_ldz2(const float *p, bool ok) { return ok ? *reinterpret_cast<const float2 *>(p) : make_float2(0.0f, 0.0f); }
__device__ __forceinline__ double cg_ldz1(const double *p, bool ok) { return ld1(p, ok); }
__device__ __forceinline__ double cg_ldz1(const float *p, bool ok) { return ok ? (double)*p : 0.0; }

// DIM 2: one row per marching step (TY = 1, no halo rows); DIM 3: TY rows and one halo row a side.  FIRST: p_new = z, p_old is not read
template <int DIM, int TY, bool FIRST, typename ZT>
__global__ void __launch_bounds__(256) k_cg_direction(const CgDirArgs a, const ZT *__restrict__ z, const double *__restrict__ po,
                                                      double *__restrict__ pn, double *__restrict__ q, double *__restrict__ parts) {
    constexpr int H = DIM == 3 ? 1 : 0, NR = TY + 2 * H;
    constexpr bool Z64 = sizeof(ZT) == 8;
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
        const long zms = Z64 ? a.ms : a.zms;
        long roff[NR], zoff[NR];
        bool rd[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) {
            roff[r] = (DIM == 3 ? (long)(i0 - H + r) * a.pitch : 0) + x0;
            zoff[r] = Z64 ? roff[r] : (DIM == 3 ? (long)(i0 - H + r) * a.zpitch : 0) + x0;
            rd[r] = on && (DIM == 2 || i0 - H + r <= a.ny);
        }
        // the wave-edge lanes' x neighbour: lane 0 column x0 - 1, lane 63 column x0 + 2 (both within the row: ghost column or interior)
        const bool edge = on && (lane == 0 || (lane == 63 && x0 + 2 <= a.nx));
        const int eoff = lane == 0 ? -1 : 2;
        double2 A[NR], B[NR], Cn[NR], pr[NR];
        typename CgPair<ZT>::type zr[NR];
#define CG_LOAD(m)                                                                                   \
        _Pragma("unroll") for (int r = 0; r < NR; r++) {                                             \
            zr[r] = cg_ldz2(z + (long)(m) * zms + zoff[r], rd[r]);                                   \
            if (!FIRST) pr[r] = ld2(po + (long)(m) * a.ms + roff[r], rd[r]);                         \
        }
#define CG_COMBINE(dst)                                                                              \
        _Pragma("unroll") for (int r = 0; r < NR; r++) {                                             \
            const double zx_ = (double)zr[r].x, zy_ = (double)zr[r].y;                               \
            if (FIRST) { dst[r].x = zx_; dst[r].y = zy_; }                                           \
            else { const double tx_ = a.beta * pr[r].x, ty_ = a.beta * pr[r].y; dst[r].x = zx_ + tx_; dst[r].y = zy_ + ty_; } \
        }
        CG_LOAD(m0 - 1) CG_COMBINE(A)
        CG_LOAD(m0) CG_COMBINE(B)
        CG_LOAD(m0 + 1)
        for (int m = m0; m < m1; m++) {
            double e[TY];
#pragma unroll
            for (int r = 0; r < TY; r++) {
                const bool ok = edge && (DIM == 2 || i0 + r < a.ny);
                const double ze = cg_ldz1(z + (long)m * zms + zoff[r + H] + eoff, ok);
                if (FIRST) e[r] = ze;
                else { const double t_ = a.beta * ld1(po + (long)m * a.ms + roff[r + H] + eoff, ok); e[r] = ze + t_; }
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

// out[0] = the n partial sums added up in a fixed order
__global__ void __launch_bounds__(256) k_cg_finish(const double *__restrict__ parts, int n, double *__restrict__ out) {
    __shared__ double red[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += parts[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

inline bool cg_geom_ok(const mgk_geom *g) {
    return g && (g->dim == 2 || g->dim == 3) && g->nx >= 1 && g->ny >= 1 && g->nz >= 1 && (g->nx & 1) && (g->dim == 3 || g->nz == 1);
}
inline int cg_capturing(hipStream_t s, bool *busy) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &st));
    *busy = st != hipStreamCaptureStatusNone;
    return 0;
}
// the partials [0, nblk) of the workspace -> result slot `slot`, its landing area, and the host if asked
inline int cg_finish(mgk_cg_ws *ws, int nblk, int slot, hipStream_t s, double *host) {
    hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(256), 0, s, ws->slots, nblk, ws->res_dev + slot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ws->land + slot, ws->res_dev + slot, sizeof(double), hipMemcpyDeviceToHost, s));
    if (host) {
        HIPCHK(hipStreamSynchronize(s));
        *host = ws->land[slot];
    }
    return 0;
}

// the launch shape of the direction pass: the arguments but the pointers, and the number of blocks (0: more blocks than the workspace has slots)
inline long cg_direction_shape(const mgk_geom *g, const double *coef, double beta, bool first, const mgk_cg_ws *ws, CgDirArgs &a) {
    memset(&a, 0, sizeof(a));
    const int ty = g->dim == 3 ? CG_TY : 1;
    a.nx = g->nx; a.ny = g->ny; a.npairs = (g->nx + 1) / 2; a.wavesx = (a.npairs + 63) / 64;
    a.nstrips = g->dim == 3 ? (g->ny + ty - 1) / ty : 1;
    a.M = g->dim == 3 ? g->nz : g->ny;
    a.pitch = g->pitch; a.ms = g->dim == 3 ? g->plane : g->pitch;
    a.zpitch = a.pitch; a.zms = a.ms;
    a.nt = store_policy();
    a.beta = first ? 0.0 : beta;
    if (g->dim == 3) set_coef7(a, coef); else set_coef5(a, coef);
    // chunks of the marching axis: enough waves to fill the chip, chunks of 32 planes or more (every chunk re-reads two halo planes),
    // never more blocks than the workspace has slots
    const long tiles = (long)a.wavesx * a.nstrips, target = 16384;
    long nch = tiles >= target ? 1 : (target + tiles - 1) / tiles;
    if (nch > (a.M + 31) / 32) nch = (a.M + 31) / 32;
    if (g_zchunk > 0) nch = (a.M + g_zchunk - 1) / g_zchunk;
    const long cap = 4L * ws->nslots / tiles;
    if (nch > cap) nch = cap;
    if (nch < 1) return 0;
    a.mlen = (int)((a.M + nch - 1) / nch);
    nch = (a.M + a.mlen - 1) / a.mlen;
    a.nwaves = tiles * nch;
    const long nblk = (a.nwaves + 3) / 4;
    return nblk > ws->nslots ? 0 : nblk;
}

}  // namespace
