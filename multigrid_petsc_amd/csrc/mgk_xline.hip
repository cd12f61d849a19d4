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
// which is line-aligned), transposed through LDS with a row pitch of 17 doubles, conflict-free in all four accesses: the tile, its lane
// struct and the bank rule are stated in mgk_line_dev.hpp.  z and u' go back the same way: lane-per-row values -> LDS -> line-wide stores.
// Tiles are loaded D steps ahead into a statically indexed register ring (the loop is unrolled by D tiles); loads and stores go through
// buffer descriptors, a row or column that must not be touched has a lane offset out of range: such a load returns 0 and such a store is
// dropped, so the ghost ring and the padding are neither read nor written.  The backward pass may write u in place (a tile is read whole
// before it is written, and no other wave touches its rows): a sweep swaps no buffers.
// Stores: as the y-line passes (mgk_store_nt_2d by size; mgk_set_tuning(variant = 0 / 1) forces one policy); the second knob (> 0) is the
// ring depth in tiles (rounded down to a built one: 1, 2, 3; default 1).
#include "mgk_line_dev.hpp"

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

// Forward.  Ring slot s holds b and g of tile t and u of tile t + 1 (the residual of a tile's last column needs the next tile's first).
template <int D, bool ZERO, bool NT>
__device__ __forceinline__ void xline_forward_body(const XLineArgs &a, double *lds) {
    const int ty = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int r0 = ty * 62 - 1;                               // row of lane 0; -1 and ny are the ghost rows (zero, not read)
    const XLane L(a.rs, a.gs, a.nx, a.ny, r0);
    const int ntile = (a.nx + XT - 1) / XT;
    double *lu = lds, *lb = lds + XTILE, *lg = lds + 2 * XTILE, *lo = lds + 3 * XTILE;
    const __amdgpu_buffer_rsrc_t wu = line_window(a.u, r0, a.rs), wb = line_window(a.b, r0, a.rs), wz = line_window(a.out, r0, a.rs),
                                 wg = line_window(a.gt, r0, a.gs);
    // the row constants of the lane's own row
    const long ri = min(max(r0 + L.lane, 0), a.ny - 1);
    double cS = 0.0, cC = 0.0, cE = 0.0, cN = 0.0;
    const double cW = a.ct[5 * ri + 1];
    if (!ZERO) { cS = a.ct[5 * ri + 0]; cC = a.ct[5 * ri + 2]; cE = a.ct[5 * ri + 3]; cN = a.ct[5 * ri + 4]; }
    double qb[D][XT], qg[D][XT], qu[D][XT];
    auto issue = [&](int t, double (&rb)[XT], double (&rg)[XT], double (&ru)[XT]) {
        const bool c0 = L.col_ok_nonneg(t), c1 = L.col_ok_nonneg(t + 1);
        const unsigned so = (unsigned)max(t, 0) * (XT * 8u);
#pragma unroll
        for (int k = 0; k < XT; k++) {
            const bool ok = L.row_ok(k);
            rb[k] = line_ld(wb, ok && c0 ? L.vf : LINE_OOB, so + (unsigned)k * L.rs8);
            rg[k] = line_ld(wg, ok && c0 ? L.vg : LINE_OOB, so + (unsigned)k * L.gs8);
            ru[k] = ZERO ? 0.0 : line_ld(wu, ok && c1 ? L.vf : LINE_OOB, so + XT * 8u + (unsigned)k * L.rs8);
        }
    };
    double uc[XT];                                            // u of the own row, the tile in hand
#pragma unroll
    for (int c = 0; c < XT; c++) uc[c] = 0.0;
    if (!ZERO) {
        const bool c0 = L.col_ok_nonneg(0);
#pragma unroll
        for (int k = 0; k < XT; k++) lu[L.rowwise(k)] = line_ld(wu, L.row_ok(k) && c0 ? L.vf : LINE_OOB, (unsigned)k * L.rs8);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int c = 0; c < XT; c++) uc[c] = lu[L.transposed(c)];
        __builtin_amdgcn_wave_barrier();
    }
    LineUnroll<0, D>::run([&](auto sc) { constexpr int s = decltype(sc)::value; issue(s, qb[s], qg[s], qu[s]); });
    double uw = 0.0, y = 0.0, gp = 0.0;
    for (int t0 = 0; t0 < ntile; t0 += D) {
        LineUnroll<0, D>::run([&](auto sc) {
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
            const bool c0 = L.col_ok_nonneg(t);
            const unsigned so = (unsigned)t * (XT * 8u);
#pragma unroll
            for (int k = 0; k < XT; k++) {
                const bool edge = (k == 0 && L.rr == 0) || (k == XT - 1 && L.rr == 3);      // tile rows 0 and 63 only supply neighbours
                line_st<NT>(lo[L.rowwise(k)], wz, L.row_ok(k) && c0 && !edge ? L.vf : LINE_OOB, so + (unsigned)k * L.rs8);
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
    const XLane L(a.rs, a.gs, a.nx, a.ny, r0);
    const int ntile = (a.nx + XT - 1) / XT;
    double *lz = lds, *lu = lds + XTILE, *lg = lds + 2 * XTILE, *lo = lds + 3 * XTILE;
    const __amdgpu_buffer_rsrc_t wz = line_window(a.z, r0, a.rs), wu = line_window(a.u, r0, a.rs), wo = line_window(a.out, r0, a.rs),
                                 wg = line_window(a.gt, r0, a.gs);
    const long ri = min(r0 + L.lane, a.ny - 1);
    const double cE = a.ct[5 * ri + 3];
    const double sc = a.scale;
    const int last = a.nx - 1;
    double qz[D][XT], qg[D][XT], qu[D][XT];
    auto issue = [&](int t, double (&rz)[XT], double (&rg)[XT], double (&ru)[XT]) {
        const bool c0 = L.col_ok_any(t);
        const unsigned so = (unsigned)max(t, 0) * (XT * 8u);
#pragma unroll
        for (int k = 0; k < XT; k++) {
            const bool ok = L.row_ok(k) && c0;
            rz[k] = line_ld(wz, ok ? L.vf : LINE_OOB, so + (unsigned)k * L.rs8);
            rg[k] = line_ld(wg, ok ? L.vg : LINE_OOB, so + (unsigned)k * L.gs8);
            ru[k] = ZERO ? 0.0 : line_ld(wu, ok ? L.vf : LINE_OOB, so + (unsigned)k * L.rs8);
        }
    };
    LineUnroll<0, D>::run([&](auto sq) { constexpr int s = decltype(sq)::value; issue(ntile - 1 - s, qz[s], qg[s], qu[s]); });
    double e = 0.0;
    for (int t0 = 0; t0 < ntile; t0 += D) {
        LineUnroll<0, D>::run([&](auto sq) {
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
            const bool c0 = L.col_ok_any(t);
            const unsigned so = (unsigned)max(t, 0) * (XT * 8u);
#pragma unroll
            for (int k = 0; k < XT; k++) line_st<NT>(lo[L.rowwise(k)], wo, L.row_ok(k) && c0 ? L.vf : LINE_OOB, so + (unsigned)k * L.rs8);
            __builtin_amdgcn_wave_barrier();
        });
    }
}

template <int D, bool ZERO>
__global__ void __launch_bounds__(64) k_xline_forward(const XLineArgs a) {
    __shared__ double lds[4 * XTILE];
    if (line_store_nt(a.nt, a.ny, a.rs)) xline_forward_body<D, ZERO, true>(a, lds); else xline_forward_body<D, ZERO, false>(a, lds);
}
template <int D, bool ZERO>
__global__ void __launch_bounds__(64) k_xline_backward(const XLineArgs a) {
    __shared__ double lds[4 * XTILE];
    if (line_store_nt(a.nt, a.ny, a.rs)) xline_backward_body<D, ZERO, true>(a, lds); else xline_backward_body<D, ZERO, false>(a, lds);
}

bool xline_geom_ok(const mgk_geom *g, long gstride) {
    return line_geom_ok(g) && (gstride == 0 || (gstride >= g->nx && gstride <= LINE_MAX_PITCH));
}
int xline_depth() { return g_zchunk >= 3 ? 3 : g_zchunk == 2 ? 2 : 1; }    // 1: the fastest at every size measured (profiles/line/README.md)
// the built ring depths, as with_depth lists them: 2 and 3 by name, 1 for everything else
template <typename F> void xline_depths(int d, F &&f) { with_depth<2, 3, 1>(d, f); }

}  // namespace

MGK_PRELOAD_UNIT(k_xline_backward<1, false>)

extern "C" int mgk_xline_forward_f64(mgk_ctx *c, const mgk_geom *g, const double *atab, const double *gtab, long gstride,
                                     const double *b, const double *u, double *z, void *stream) {
    if (!c || !xline_geom_ok(g, gstride) || !atab || !gtab || !b || !z || z == b || z == u)
        return fail(MGK_EINVAL, "mgk_xline_forward_f64: bad arguments (2-D; z must not alias b or u; gstride 0 or >= nx)");
    XLineArgs a; memset(&a, 0, sizeof(a));
    a.u = u ? u + g->org : nullptr; a.b = b + g->org; a.out = z + g->org;
    a.ct = atab; a.gt = gtab; a.gs = gstride;
    a.nx = g->nx; a.ny = g->ny; a.rs = g->pitch; a.nt = store_policy();
    const dim3 grid((unsigned)((g->ny + 61) / 62));
    LAUNCH_DEPTH_ZERO(xline_depths, xline_depth(), u == nullptr, k_xline_forward, grid, S(c, stream), a);
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
    LAUNCH_DEPTH_ZERO(xline_depths, xline_depth(), u == nullptr, k_xline_backward, grid, S(c, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}
