// mgk_xline.hip -- x-line Jacobi on the 2-D row-table operators: one sweep u <- u + s T_x^-1 (b - A u), T_x = the
// x-tridiagonal part of A.  In row i it is the constant-band matrix (W_i, C_i, E_i); its factorisation along the columns j is ONE table
// made on the host (mg_xline.c): g_{i,j} = 1 / pivot.  The multipliers l_{i,j} = W_i g_{i,j-1} (l_{i,0} = 0) and q_{i,j} = E_i g_{i,j} are
// one rounded product each of a table value and a row constant, formed here.
//   mgk_xline_forward_f64    r = b - A u (five terms in the order of mgk_rowcoef_f64 mode 1; from the zero guess r = b, u is not read)
//                            y_{i,0} = r_{i,0}, y_{i,j} = r_{i,j} - l_{i,j} y_{i,j-1};  z_{i,j} = y_{i,j} g_{i,j}, stored     32 B per unknown (zero guess: 24)
//   mgk_xline_backward_f64   e_{i,n-1} = z_{i,n-1}, e_{i,j} = z_{i,j} - q_{i,j} e_{i,j+1};  u' = u + s e (zero guess: s e)     32 B per unknown (24)
// (on the uniform mesh g is one row of n doubles, row stride 0, and stays in cache: 24 / 16 and 24 / 16.)
// fp64, no FMA (-ffp-contract=off).  The recurrence runs ALONG a row, so a lane owns a ROW and the wave marches over all columns: left to
// right in the forward pass, right to left in the backward pass.  Every wave is a block of its own (no barrier, its own LDS).  Forward:
// lane l of wave ty holds row 62 ty + l - 1, the y neighbours of u come by DPP wave shifts, lanes 1 .. 62 store (tiles overlap by two
// rows).  Backward: a point reads only itself, 64 rows per wave.
// Memory stays coalesced: a step moves a TILE of 64 rows x 16 columns, one whole 128-byte line per row (interior column 0 sits at MGK_XOFF,
// which is line-aligned), four rows per load instruction: lane (rr, cc) = (lane / 16, lane % 16) of load k moves row 16 rr + k, column cc.
// The tile is transposed through LDS with a row pitch of 17 doubles.  By the bank rule of the 8-byte LDS accesses -- ds_read_b64: two
// groups of 32 lanes, bank pair (a / 8) mod 32; ds_write_b64: four groups of 16 contiguous lanes, bank pair (a / 8) mod 16 -- all four
// accesses are conflict-free: row-wise write and read touch (272 rr + 17 k + cc), 16 consecutive doubles per group of 16 lanes and, as
// 272 = 16 (mod 32), 32 consecutive ones per half wave; the transposed read and write touch (17 lane + c), distinct mod 32 in a half wave
// and mod 16 in 16 contiguous lanes because 17 is odd.  z and u' go back the same way: lane-per-row values -> LDS -> line-wide stores.
// Tiles are loaded D steps ahead into a statically indexed register ring (the loop is unrolled by D tiles); loads and stores go through
// buffer descriptors, a row or column that must not be touched has a lane offset out of range: such a load returns 0 and such a store is
// dropped, so the ghost ring and the padding are neither read nor written.  The backward pass may write u in place (a tile is read whole
// before it is written, and no other wave touches its rows): a sweep swaps no buffers.
// Stores: as the y-line passes (mgk_store_nt_2d by size; mgk_set_tuning(variant = 0 / 1) forces one policy); the second knob (> 0) is the
// ring depth in tiles (rounded down to a built one: 1, 2, 3; default 1).
#include "mgk_dev.hpp"
#include <type_traits>

namespace {

struct XLineArgs {
    const double *u, *b, *z;        // forward: u (unused from the zero guess), b; backward: z, u (unused from the zero guess)
    double *out;                    // forward: z; backward: unew
    const double *ct, *gt;          // the row table (ny x 5) and g (row stride gs; 0: one row for every grid row)
    int nx, ny;
    long rs, gs;
    double scale;
    int nt;                         // store policy: < 0 by size, 0 ordinary, 1 non-temporal
};

constexpr int XT = 16;                          // columns per tile: one 128-byte line per row
constexpr int XP = XT + 1;                      // LDS row pitch in doubles (odd: see the bank rule above)
constexpr int XTILE = 64 * XP;                  // doubles of one tile in LDS
constexpr int XL_RECORDS = 0x7ffffff0;          // every buffer window: far more than a window spans (the host checks the pitch) ...
constexpr unsigned XL_OOB = 0x7ffffff8u;        // ... and below the lane offset of a lane that must not load or store
constexpr long XL_MAX_PITCH = 1L << 21;         // 64 rows of a window and a row of 2^21 doubles stay below 2^31 bytes

typedef unsigned int xl_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bool xl_nt(const XLineArgs &a) { return a.nt < 0 ? mgk_store_nt_2d(a.ny, a.rs) : a.nt != 0; }
// a window of a field or of the table: row `row`, column 0 at offset 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t xl_window(const double *p, long row, long rs) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)((uintptr_t)p + (uintptr_t)(row * rs * 8)), 0, XL_RECORDS, 0x00020000);
}
__device__ __forceinline__ double xl_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
template <bool NT> __device__ __forceinline__ void xl_st(double v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(xl_u2, v), r, voff, soff, NT ? 2 : 0);
}
template <int K, int N> struct XlUnroll {
    template <class F> static __device__ __forceinline__ void run(F &&f) { f(std::integral_constant<int, K>{}); XlUnroll<K + 1, N>::run(f); }
};
template <int N> struct XlUnroll<N, N> { template <class F> static __device__ __forceinline__ void run(F &&) {} };

// what both passes know about their lane: in the row-wise form of a tile lane (rr, cc) moves row r0 + 16 rr + k with load / store k
struct XlLane {
    int lane, rr, cc, rq;           // rq: the row of load 0
    unsigned vf, vg;                // lane offsets (bytes) into a field window and into the table window
    unsigned rs8, gs8;
    int nx, ny;
    __device__ __forceinline__ XlLane(const XLineArgs &a, int r0) {
        lane = threadIdx.x; rr = lane >> 4; cc = lane & 15; rq = r0 + 16 * rr;
        vf = (unsigned)((16 * rr * a.rs + cc) * 8); vg = (unsigned)((16 * rr * a.gs + cc) * 8);
        rs8 = (unsigned)a.rs * 8u; gs8 = (unsigned)a.gs * 8u;
        nx = a.nx; ny = a.ny;
    }
    __device__ __forceinline__ bool row_ok(int k) const { return (unsigned)(rq + k) < (unsigned)ny; }      // a grid row (not a ghost row)
    __device__ __forceinline__ bool col_ok(int t) const { return t >= 0 && t * XT + cc < nx; }              // an interior column of tile t
    __device__ __forceinline__ int rowwise(int k) const { return (16 * rr + k) * XP + cc; }                 // LDS index, row-wise form
    __device__ __forceinline__ int transposed(int c) const { return lane * XP + c; }                        // LDS index, lane-per-row form
};

// Forward.  Ring slot s holds b and g of tile t and u of tile t + 1 (the residual of a tile's last column needs the next tile's first).
template <int D, bool ZERO, bool NT>
__device__ __forceinline__ void xline_forward_body(const XLineArgs &a, double *lds) {
    const int ty = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int r0 = ty * 62 - 1;                               // row of lane 0; -1 and ny are the ghost rows (zero, not read)
    const XlLane L(a, r0);
    const int ntile = (a.nx + XT - 1) / XT;
    double *lu = lds, *lb = lds + XTILE, *lg = lds + 2 * XTILE, *lo = lds + 3 * XTILE;
    const __amdgpu_buffer_rsrc_t wu = xl_window(a.u, r0, a.rs), wb = xl_window(a.b, r0, a.rs), wz = xl_window(a.out, r0, a.rs),
                                 wg = xl_window(a.gt, r0, a.gs);
    // the row constants of the lane's own row
    const long ri = min(max(r0 + L.lane, 0), a.ny - 1);
    double cS = 0.0, cC = 0.0, cE = 0.0, cN = 0.0;
    const double cW = a.ct[5 * ri + 1];
    if (!ZERO) { cS = a.ct[5 * ri + 0]; cC = a.ct[5 * ri + 2]; cE = a.ct[5 * ri + 3]; cN = a.ct[5 * ri + 4]; }
    double qb[D][XT], qg[D][XT], qu[D][XT];
    auto issue = [&](int t, double (&rb)[XT], double (&rg)[XT], double (&ru)[XT]) {
        const bool c0 = L.col_ok(t), c1 = L.col_ok(t + 1);
        const unsigned so = (unsigned)max(t, 0) * (XT * 8u);
#pragma unroll
        for (int k = 0; k < XT; k++) {
            const bool ok = L.row_ok(k);
            rb[k] = xl_ld(wb, ok && c0 ? L.vf : XL_OOB, so + (unsigned)k * L.rs8);
            rg[k] = xl_ld(wg, ok && c0 ? L.vg : XL_OOB, so + (unsigned)k * L.gs8);
            ru[k] = ZERO ? 0.0 : xl_ld(wu, ok && c1 ? L.vf : XL_OOB, so + XT * 8u + (unsigned)k * L.rs8);
        }
    };
    double uc[XT];                                            // u of the own row, the tile in hand
#pragma unroll
    for (int c = 0; c < XT; c++) uc[c] = 0.0;
    if (!ZERO) {
        const bool c0 = L.col_ok(0);
#pragma unroll
        for (int k = 0; k < XT; k++) lu[L.rowwise(k)] = xl_ld(wu, L.row_ok(k) && c0 ? L.vf : XL_OOB, (unsigned)k * L.rs8);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int c = 0; c < XT; c++) uc[c] = lu[L.transposed(c)];
        __builtin_amdgcn_wave_barrier();
    }
    XlUnroll<0, D>::run([&](auto sc) { constexpr int s = decltype(sc)::value; issue(s, qb[s], qg[s], qu[s]); });
    double uw = 0.0, y = 0.0, gp = 0.0;
    for (int t0 = 0; t0 < ntile; t0 += D) {
        XlUnroll<0, D>::run([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            const int t = t0 + s;                             // t >= ntile: computes on zeros, stores nothing
#pragma unroll
            for (int k = 0; k < XT; k++) {
                lb[L.rowwise(k)] = qb[s][k];
                lg[L.rowwise(k)] = qg[s][k];
                if (!ZERO) lu[L.rowwise(k)] = qu[s][k];
            }
            issue(t + D, qb[s], qg[s], qu[s]);
            __builtin_amdgcn_wave_barrier();
            double bt[XT], gt[XT], un[XT];
#pragma unroll
            for (int c = 0; c < XT; c++) {
                bt[c] = lb[L.transposed(c)];
                gt[c] = lg[L.transposed(c)];
                un[c] = ZERO ? 0.0 : lu[L.transposed(c)];
            }
#pragma unroll
            for (int c = 0; c < XT; c++) {
                double r = bt[c];
                if (!ZERO) {
                    const double um = uc[c], ue = c + 1 < XT ? uc[c + 1] : un[0];
                    const double sv = lane_up<true>(um), nv = lane_dn<true>(um);
                    double q = cS * sv;
                    q = q + cW * uw;
                    q = q + cC * um;
                    q = q + cE * ue;
                    q = q + cN * nv;
                    r = bt[c] - q;
                    uw = um;
                }
                double l = cW * gp;
                if (c == 0) l = t == 0 ? 0.0 : l;             // l_{i,0} = 0
                const double ly = l * y;
                y = r - ly;
                gp = gt[c];
                lo[L.transposed(c)] = y * gp;
            }
            if (!ZERO) {
#pragma unroll
                for (int c = 0; c < XT; c++) uc[c] = un[c];
            }
            __builtin_amdgcn_wave_barrier();
            const bool c0 = L.col_ok(t);
            const unsigned so = (unsigned)t * (XT * 8u);
#pragma unroll
            for (int k = 0; k < XT; k++) {
                const bool edge = (k == 0 && L.rr == 0) || (k == XT - 1 && L.rr == 3);      // tile rows 0 and 63 only supply neighbours
                xl_st<NT>(lo[L.rowwise(k)], wz, L.row_ok(k) && c0 && !edge ? L.vf : XL_OOB, so + (unsigned)k * L.rs8);
            }
            __builtin_amdgcn_wave_barrier();
        });
    }
}

// Backward: tiles from the right, ring slot s holds z, g and u of tile ntile - 1 - tt, tt = s (mod D).
template <int D, bool ZERO, bool NT>
__device__ __forceinline__ void xline_backward_body(const XLineArgs &a, double *lds) {
    const int ty = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int r0 = ty * 64;
    const XlLane L(a, r0);
    const int ntile = (a.nx + XT - 1) / XT;
    double *lz = lds, *lu = lds + XTILE, *lg = lds + 2 * XTILE, *lo = lds + 3 * XTILE;
    const __amdgpu_buffer_rsrc_t wz = xl_window(a.z, r0, a.rs), wu = xl_window(a.u, r0, a.rs), wo = xl_window(a.out, r0, a.rs),
                                 wg = xl_window(a.gt, r0, a.gs);
    const long ri = min(r0 + L.lane, a.ny - 1);
    const double cE = a.ct[5 * ri + 3];
    const double sc = a.scale;
    const int last = a.nx - 1;
    double qz[D][XT], qg[D][XT], qu[D][XT];
    auto issue = [&](int t, double (&rz)[XT], double (&rg)[XT], double (&ru)[XT]) {
        const bool c0 = L.col_ok(t);
        const unsigned so = (unsigned)max(t, 0) * (XT * 8u);
#pragma unroll
        for (int k = 0; k < XT; k++) {
            const bool ok = L.row_ok(k) && c0;
            rz[k] = xl_ld(wz, ok ? L.vf : XL_OOB, so + (unsigned)k * L.rs8);
            rg[k] = xl_ld(wg, ok ? L.vg : XL_OOB, so + (unsigned)k * L.gs8);
            ru[k] = ZERO ? 0.0 : xl_ld(wu, ok ? L.vf : XL_OOB, so + (unsigned)k * L.rs8);
        }
    };
    XlUnroll<0, D>::run([&](auto sq) { constexpr int s = decltype(sq)::value; issue(ntile - 1 - s, qz[s], qg[s], qu[s]); });
    double e = 0.0;
    for (int t0 = 0; t0 < ntile; t0 += D) {
        XlUnroll<0, D>::run([&](auto sq) {
            constexpr int s = decltype(sq)::value;
            const int t = ntile - 1 - (t0 + s);               // t < 0: computes on zeros, stores nothing
#pragma unroll
            for (int k = 0; k < XT; k++) {
                lz[L.rowwise(k)] = qz[s][k];
                lg[L.rowwise(k)] = qg[s][k];
                if (!ZERO) lu[L.rowwise(k)] = qu[s][k];
            }
            issue(t - D, qz[s], qg[s], qu[s]);
            __builtin_amdgcn_wave_barrier();
            double zt[XT], gt[XT], ut[XT];
#pragma unroll
            for (int c = 0; c < XT; c++) {
                zt[c] = lz[L.transposed(c)];
                gt[c] = lg[L.transposed(c)];
                ut[c] = ZERO ? 0.0 : lu[L.transposed(c)];
            }
#pragma unroll
            for (int c = XT - 1; c >= 0; c--) {
                const double q = cE * gt[c];
                double qe = q * e;
                qe = t * XT + c >= last ? 0.0 : qe;           // e_{i,n-1} = z_{i,n-1}; the columns past it hold zeros
                e = zt[c] - qe;
                const double se = sc * e;
                lo[L.transposed(c)] = ZERO ? se : ut[c] + se;
            }
            __builtin_amdgcn_wave_barrier();
            const bool c0 = L.col_ok(t);
            const unsigned so = (unsigned)max(t, 0) * (XT * 8u);
#pragma unroll
            for (int k = 0; k < XT; k++) xl_st<NT>(lo[L.rowwise(k)], wo, L.row_ok(k) && c0 ? L.vf : XL_OOB, so + (unsigned)k * L.rs8);
            __builtin_amdgcn_wave_barrier();
        });
    }
}

template <int D, bool ZERO>
__global__ void __launch_bounds__(64) k_xline_forward(const XLineArgs a) {
    __shared__ double lds[4 * XTILE];
    if (xl_nt(a)) xline_forward_body<D, ZERO, true>(a, lds); else xline_forward_body<D, ZERO, false>(a, lds);
}
template <int D, bool ZERO>
__global__ void __launch_bounds__(64) k_xline_backward(const XLineArgs a) {
    __shared__ double lds[4 * XTILE];
    if (xl_nt(a)) xline_backward_body<D, ZERO, true>(a, lds); else xline_backward_body<D, ZERO, false>(a, lds);
}

bool xline_geom_ok(const mgk_geom *g, long gstride) {
    return g && g->dim == 2 && g->nz == 1 && g->nx >= 1 && g->ny >= 1 && g->pitch <= XL_MAX_PITCH && (gstride == 0 || (gstride >= g->nx && gstride <= XL_MAX_PITCH));
}
int xline_depth() { return g_zchunk >= 3 ? 3 : g_zchunk == 2 ? 2 : 1; }    // 1: the fastest at every size measured (profiles/line/README.md)

}  // namespace

int mgk_preload_xline() {
    hipFuncAttributes fa;
    HIPCHK(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_xline_backward<1, false>)));
    return 0;
}

#define XLINE_DISPATCH(KERNEL, zero, grid, s, a)                                                             \
    do {                                                                                                     \
        const int d_ = xline_depth();                                                                        \
        if (zero) {                                                                                          \
            if (d_ == 2) hipLaunchKernelGGL((KERNEL<2, true>), grid, dim3(64), 0, s, a);                     \
            else if (d_ == 3) hipLaunchKernelGGL((KERNEL<3, true>), grid, dim3(64), 0, s, a);                \
            else hipLaunchKernelGGL((KERNEL<1, true>), grid, dim3(64), 0, s, a);                             \
        } else {                                                                                             \
            if (d_ == 2) hipLaunchKernelGGL((KERNEL<2, false>), grid, dim3(64), 0, s, a);                    \
            else if (d_ == 3) hipLaunchKernelGGL((KERNEL<3, false>), grid, dim3(64), 0, s, a);               \
            else hipLaunchKernelGGL((KERNEL<1, false>), grid, dim3(64), 0, s, a);                            \
        }                                                                                                    \
    } while (0)

extern "C" int mgk_xline_forward_f64(mgk_ctx *c, const mgk_geom *g, const double *atab, const double *gtab, long gstride,
                                     const double *b, const double *u, double *z, void *stream) {
    if (!c || !xline_geom_ok(g, gstride) || !atab || !gtab || !b || !z || z == b || z == u)
        return fail(MGK_EINVAL, "mgk_xline_forward_f64: bad arguments (2-D; z must not alias b or u; gstride 0 or >= nx)");
    XLineArgs a; memset(&a, 0, sizeof(a));
    a.u = u ? u + g->org : nullptr; a.b = b + g->org; a.out = z + g->org;
    a.ct = atab; a.gt = gtab; a.gs = gstride;
    a.nx = g->nx; a.ny = g->ny; a.rs = g->pitch; a.nt = store_policy();
    const dim3 grid((unsigned)((g->ny + 61) / 62));
    XLINE_DISPATCH(k_xline_forward, u == nullptr, grid, S(c, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mgk_xline_backward_f64(mgk_ctx *c, const mgk_geom *g, const double *atab, const double *gtab, long gstride, double scale,
                                      const double *z, const double *u, double *unew, void *stream) {
    if (!c || !xline_geom_ok(g, gstride) || !atab || !gtab || !z || !unew || unew == z)
        return fail(MGK_EINVAL, "mgk_xline_backward_f64: bad arguments (2-D; unew must not alias z; gstride 0 or >= nx)");
    XLineArgs a; memset(&a, 0, sizeof(a));
    a.z = z + g->org; a.u = u ? u + g->org : nullptr; a.out = unew + g->org;
    a.ct = atab; a.gt = gtab; a.gs = gstride;
    a.nx = g->nx; a.ny = g->ny; a.rs = g->pitch; a.scale = scale; a.nt = store_policy();
    const dim3 grid((unsigned)((g->ny + 63) / 64));
    XLINE_DISPATCH(k_xline_backward, u == nullptr, grid, S(c, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}
