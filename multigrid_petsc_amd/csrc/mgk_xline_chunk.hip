// mgk_xline_chunk.hip -- the x-line sweep of mgk_xline.hip with its tridiagonal systems solved in chunks (the definition
// and the tables: include/mgk.h, csrc/mg_xline_chunk.c): period c, a multiple of 16, K = nx / c, column s_q = q c + c - 1 is separator q, the
// columns [k c, min(k c + c - 1, nx)) are chunk k.  The Thomas recurrence is serial along x and a lane owns a row, so the plain passes run on
// ny / 62 waves whatever the width; here every chunk is a wave of its own, (K + 1) times as many.  Four passes over one scratch field t and a
// separator workspace sep of four planes R, XL, XR, XI of K rows of ss = ny rounded up to 16 doubles (element (p, q, i) at
// sep[(p K + q) ss + i]): what the separator system needs of a row, written and read by the lane that owns the row -- coalesced, where a read
// of a column of t would touch 64 lines per load:
//   mgk_xline_chunk_forward_f64    one wave per (62-row tile, chunk): k_xline_forward's march restarted at the chunk's first column (u west of
//                                  it is one column load); t = y g, the separator east of the chunk gets its r_s, in t and in R
//   mgk_xline_chunk_backward_f64   one wave per (64-row tile, chunk): the back substitution, t -> x' in place; x' of the chunk's two end columns
//                                  goes to XL (of the separator east of it) and XR (of the separator west of it)
//   mgk_xline_chunk_reduce_f64     a lane owns a row and marches over the K separators: rho_q from R, XL, XR, down (Z_q kept in XI), then up
//                                  (xi_q over it); the loads of the next four separators are issued ahead of the four in hand
//   mgk_xline_chunk_correct_f64    streaming: a lane owns an aligned column pair (16-byte accesses), a wave up to 128 columns of up to 16 rows
//                                  of ONE chunk, so that xi of the two separators around it is wave-uniform (scalar loads) and v, w of a
//                                  stride-0 table are loaded once; x = (x' - xi_{k-1} v) - xi_k w, u' = u + s x
// fp64, no FMA (-ffp-contract=off).  Every wave is a block of its own; the chunk comes from blockIdx through readfirstlane.  The two marches
// move tiles of 64 rows x 16 columns, one 128-byte line per row, transposed through the wave's own LDS at a pitch of 17 doubles, through
// buffer descriptors: mgk_xline.hip's scheme (the bank rule and the out-of-range lane offset are stated in mgk_line_dev.hpp) with a ring of one tile.  c is
// a multiple of 16, so a chunk starts on a line, is a whole number of tiles, and its separator is the last column of its last tile.
// Nothing outside the interior of an output is written; neither the ghost ring nor the padding of an input is read; an entry of sep the
// definition never forms is neither written nor read.  Stores: mgk_store_nt_2d, or the policy mgk_set_tuning(0 / 1) forces.
#include "mgk_line_dev.hpp"

namespace {

struct XChunkArgs {
    const double *u, *b;            // forward: u (unused from the zero guess), b; correct: u (unused from the zero guess)
    double *t;                      // the scratch field: forward writes it, backward updates it in place, correct reads it
    double *sep;                    // the separator workspace
    double *out;                    // correct: unew
    const double *ct;               // the row table (ny x 5)
    const double *t0, *t1, *t2;     // forward, backward: g; reduce: SL, SG, SQ; correct: v, w
    int nx, ny, c, K;
    long rs, gs, ss;                // row strides of the fields, of the tables (gs; reduce: of SL, SG, SQ) and of sep
    double scale;
    int nt;                         // store policy: < 0 by size, 0 ordinary, 1 non-temporal
};

constexpr int XC_S = 4;                         // reduce: separators whose loads are in flight together
constexpr int XC_R = 8;                         // correct: rows whose loads are in flight together ...
constexpr int XC_ROWS = 16;                     // ... and rows of a wave

// Forward, chunk k: the tiles [tb, te), the separator (k < K) the last column of tile te - 1.  The ring slot holds b and g of tile t and u of
// tile t + 1 (the residual of a tile's last column needs the next tile's first -- at the separator the next chunk's first column).
template <bool ZERO, bool NT>
__device__ __forceinline__ void xchunk_forward_body(const XChunkArgs &a, double *lds) {
    const int ty = __builtin_amdgcn_readfirstlane(blockIdx.x), k = __builtin_amdgcn_readfirstlane(blockIdx.y);
    const int r0 = ty * 62 - 1;                               // row of lane 0; -1 and ny are the ghost rows (zero, not read)
    const XLane L(a.rs, a.gs, a.nx, a.ny, r0);
    const int ntile = (a.nx + XT - 1) / XT;
    const bool hassep = k < a.K;
    const int tb = k * (a.c / XT), te = hassep ? tb + a.c / XT : ntile;
    double *lu = lds, *lb = lds + XTILE, *lg = lds + 2 * XTILE, *lo = lds + 3 * XTILE;
    const __amdgpu_buffer_rsrc_t wu = line_window(a.u, r0, a.rs), wb = line_window(a.b, r0, a.rs), wz = line_window(a.t, r0, a.rs),
                                 wg = line_window(a.t0, r0, a.gs);
    const int row = r0 + L.lane;
    const bool mine = L.lane >= 1 && L.lane <= 62 && row < a.ny;       // a row this lane stores
    const long ri = min(max(row, 0), a.ny - 1);
    double cS = 0.0, cC = 0.0, cE = 0.0, cN = 0.0;
    const double cW = a.ct[5 * ri + 1];
    if (!ZERO) { cS = a.ct[5 * ri + 0]; cC = a.ct[5 * ri + 2]; cE = a.ct[5 * ri + 3]; cN = a.ct[5 * ri + 4]; }
    double qb[XT], qg[XT], qu[XT];
    auto issue = [&](int t) {                                 // t >= te: nothing is loaded
        const bool c0 = t < te && L.col_ok_nonneg(t), c1 = t < te && L.col_ok_nonneg(t + 1);
        const unsigned so = (unsigned)t * (XT * 8u);
#pragma unroll
        for (int q = 0; q < XT; q++) {
            const bool ok = L.row_ok(q);
            qb[q] = line_ld(wb, ok && c0 ? L.vf : LINE_OOB, so + (unsigned)q * L.rs8);
            qg[q] = line_ld(wg, ok && c0 ? L.vg : LINE_OOB, so + (unsigned)q * L.gs8);
            qu[q] = ZERO ? 0.0 : line_ld(wu, ok && c1 ? L.vf : LINE_OOB, so + XT * 8u + (unsigned)q * L.rs8);
        }
    };
    double uc[XT];                                            // u of the own row, the tile in hand
    double uw = 0.0;                                          // ... and of the column west of it (the ghost column for chunk 0)
#pragma unroll
    for (int c = 0; c < XT; c++) uc[c] = 0.0;
    if (!ZERO) {
        const bool c0 = L.col_ok_nonneg(tb);
        const unsigned so = (unsigned)tb * (XT * 8u);
#pragma unroll
        for (int q = 0; q < XT; q++) lu[L.rowwise(q)] = line_ld(wu, L.row_ok(q) && c0 ? L.vf : LINE_OOB, so + (unsigned)q * L.rs8);
        if (k > 0 && (unsigned)row < (unsigned)a.ny) uw = a.u[(long)row * a.rs + (long)tb * XT - 1];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int c = 0; c < XT; c++) uc[c] = lu[L.transposed(c)];
        __builtin_amdgcn_wave_barrier();
    }
    issue(tb);
    double y = 0.0, gp = 0.0, rsep = 0.0;
    for (int t = tb; t < te; t++) {
#pragma unroll
        for (int q = 0; q < XT; q++) {
            lb[L.rowwise(q)] = qb[q];
            lg[L.rowwise(q)] = qg[q];
            if (!ZERO) lu[L.rowwise(q)] = qu[q];
        }
        issue(t + 1);
        __builtin_amdgcn_wave_barrier();
        double bt[XT], gt[XT], un[XT];
#pragma unroll
        for (int c = 0; c < XT; c++) {
            bt[c] = lb[L.transposed(c)];
            gt[c] = lg[L.transposed(c)];
            un[c] = ZERO ? 0.0 : lu[L.transposed(c)];
        }
        const bool septile = hassep && t == te - 1;
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
            if (c == 0) l = t == tb ? 0.0 : l;                // l = 0 at the chunk's first column
            const double ly = l * y;
            y = r - ly;
            gp = gt[c];
            double o = y * gp;
            if (c == XT - 1) {                                // the separator keeps its residual
                o = septile ? r : o;
                rsep = r;
            }
            lo[L.transposed(c)] = o;
        }
        if (!ZERO) {
#pragma unroll
            for (int c = 0; c < XT; c++) uc[c] = un[c];
        }
        __builtin_amdgcn_wave_barrier();
        const bool c0 = L.col_ok_nonneg(t);
        const unsigned so = (unsigned)t * (XT * 8u);
#pragma unroll
        for (int q = 0; q < XT; q++) {
            const bool edge = (q == 0 && L.rr == 0) || (q == XT - 1 && L.rr == 3);      // tile rows 0 and 63 only supply neighbours
            line_st<NT>(lo[L.rowwise(q)], wz, L.row_ok(q) && c0 && !edge ? L.vf : LINE_OOB, so + (unsigned)q * L.rs8);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (hassep && mine) a.sep[(long)k * a.ss + row] = rsep;   // R[k]
}

// Backward, chunk k = the columns [ca, cb): tiles from the right, the ring slot holds z and g of the tile.
template <bool NT>
__device__ __forceinline__ void xchunk_backward_body(const XChunkArgs &a, double *lds) {
    const int ty = __builtin_amdgcn_readfirstlane(blockIdx.x), k = __builtin_amdgcn_readfirstlane(blockIdx.y);
    const int r0 = ty * 64;
    const XLane L(a.rs, a.gs, a.nx, a.ny, r0);
    const int ntile = (a.nx + XT - 1) / XT;
    const bool hassep = k < a.K;
    const int tb = k * (a.c / XT), te = hassep ? tb + a.c / XT : ntile;
    const int cb = hassep ? k * a.c + a.c - 1 : a.nx;         // one past the chunk's last column
    double *lz = lds, *lg = lds + XTILE, *lo = lds + 2 * XTILE;
    const __amdgpu_buffer_rsrc_t wz = line_window(a.t, r0, a.rs), wg = line_window(a.t0, r0, a.gs);
    const int row = r0 + L.lane;
    const long ri = min(row, a.ny - 1);
    const double cE = a.ct[5 * ri + 3];
    double qz[XT], qg[XT];
    auto issue = [&](int t) {                                 // t < tb: nothing is loaded
        const bool c0 = t >= tb && L.col_ok_nonneg(t);
        const unsigned so = (unsigned)max(t, 0) * (XT * 8u);
#pragma unroll
        for (int q = 0; q < XT; q++) {
            const bool ok = L.row_ok(q) && c0;
            qz[q] = line_ld(wz, ok ? L.vf : LINE_OOB, so + (unsigned)q * L.rs8);
            qg[q] = line_ld(wg, ok ? L.vg : LINE_OOB, so + (unsigned)q * L.gs8);
        }
    };
    issue(te - 1);
    double e = 0.0, xl = 0.0;
    for (int t = te - 1; t >= tb; t--) {
#pragma unroll
        for (int q = 0; q < XT; q++) {
            lz[L.rowwise(q)] = qz[q];
            lg[L.rowwise(q)] = qg[q];
        }
        issue(t - 1);
        __builtin_amdgcn_wave_barrier();
        double zt[XT], gt[XT];
#pragma unroll
        for (int c = 0; c < XT; c++) {
            zt[c] = lz[L.transposed(c)];
            gt[c] = lg[L.transposed(c)];
        }
        const bool septile = hassep && t == te - 1;
#pragma unroll
        for (int c = XT - 1; c >= 0; c--) {
            const double q = cE * gt[c];
            double qe = q * e;
            qe = t * XT + c >= cb - 1 ? 0.0 : qe;             // x'_{b-1} = z_{b-1}; the separator column and the columns past nx pass through
            e = zt[c] - qe;
            if (c == XT - 2) xl = septile ? e : xl;           // x' west of the separator
            lo[L.transposed(c)] = e;
        }
        __builtin_amdgcn_wave_barrier();
        const bool c0 = L.col_ok_nonneg(t) && !(septile && L.cc == XT - 1);   // the separator column stays
        const unsigned so = (unsigned)t * (XT * 8u);
#pragma unroll
        for (int q = 0; q < XT; q++) line_st<NT>(lo[L.rowwise(q)], wz, L.row_ok(q) && c0 ? L.vf : LINE_OOB, so + (unsigned)q * L.rs8);
        __builtin_amdgcn_wave_barrier();
    }
    if (row < a.ny) {
        if (hassep) a.sep[((long)a.K + k) * a.ss + row] = xl;              // XL[k]
        if (k > 0) a.sep[(2L * a.K + k - 1) * a.ss + row] = e;             // XR[k - 1]: x' of the chunk's first column
    }
}

__device__ __forceinline__ void xchunk_reduce_body(const XChunkArgs &a) {
    const int lane = threadIdx.x;
    const int tx = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int K = a.K;
    const long ss = a.ss, st = a.gs ? a.gs : 1;               // sstride 0: one value per separator for every row, entry [q]
    const int row = tx * 64 + lane;
    if (row >= a.ny) return;
    const double *R = a.sep + row, *XL = R + (long)K * ss, *XR = XL + (long)K * ss;
    double *XI = a.sep + 3L * K * ss + row;
    const long ti = a.gs ? row : 0;
    const double *SL = a.t0 + ti, *SG = a.t1 + ti, *SQ = a.t2 + ti;
    const double cW = a.ct[5L * row + 1], cE = a.ct[5L * row + 3];
    const bool lastright = a.nx > K * a.c;                    // a column east of the last separator: XR[K - 1] exists
    // both marches are software-pipelined as mgk_line_chunk.hip's: the loads of the NEXT XC_S separators are issued before the serial
    // recurrence of the XC_S in hand
    double Y = 0.0, Z = 0.0;
    double xm[XC_S], x0[XC_S], xp[XC_S], sl[XC_S], sg[XC_S], nm[XC_S], n0[XC_S], np[XC_S], nl[XC_S], ng[XC_S];
    auto load_down = [&](int q0, double *am, double *a0, double *ap, double *al, double *ag) {
#pragma unroll
        for (int j = 0; j < XC_S; j++) {
            const int q = min(q0 + j, K - 1);
            am[j] = XL[q * ss];
            a0[j] = R[q * ss];
            ap[j] = (q < K - 1 || lastright) ? XR[q * ss] : 0.0;
            al[j] = SL[q * st];
            ag[j] = SG[q * st];
        }
    };
    load_down(0, xm, x0, xp, sl, sg);
    for (int q0 = 0; q0 < K; q0 += XC_S) {                    // down: Z_q into XI[q]
        load_down(q0 + XC_S, nm, n0, np, nl, ng);             // (past the last separator: clamped, unused)
#pragma unroll
        for (int j = 0; j < XC_S; j++) {
            const int q = q0 + j;
            if (q < K) {                                      // (wave-uniform)
                double t = cW * xm[j];
                double rho = x0[j] - t;
                if (q < K - 1 || lastright) {
                    t = cE * xp[j];
                    rho = rho - t;
                }
                if (q == 0) Y = rho;
                else {
                    t = sl[j] * Y;
                    Y = rho - t;
                }
                Z = Y * sg[j];
                XI[q * ss] = Z;
            }
        }
#pragma unroll
        for (int j = 0; j < XC_S; j++) { xm[j] = nm[j]; x0[j] = n0[j]; xp[j] = np[j]; sl[j] = nl[j]; sg[j] = ng[j]; }
    }
    double xi = Z;                                            // xi_{K-1} = Z_{K-1}: already in place
    auto load_up = [&](int q0, double *az, double *aq) {
#pragma unroll
        for (int j = 0; j < XC_S; j++) {
            const int q = max(q0 - j, 0);
            az[j] = XI[q * ss];                               // (this lane's own stores of the march down)
            aq[j] = SQ[q * st];
        }
    };
    load_up(K - 2, x0, sl);
    for (int q0 = K - 2; q0 >= 0; q0 -= XC_S) {               // up: xi_q over Z_q
        load_up(q0 - XC_S, n0, nl);
#pragma unroll
        for (int j = 0; j < XC_S; j++) {
            const int q = q0 - j;
            if (q >= 0) {
                const double t = sl[j] * xi;
                xi = x0[j] - t;
                XI[q * ss] = xi;
            }
        }
#pragma unroll
        for (int j = 0; j < XC_S; j++) { x0[j] = n0[j]; sl[j] = nl[j]; }
    }
}

template <bool ZERO, bool NT>
__device__ __forceinline__ void xchunk_correct_body(const XChunkArgs &a, int pieces) {
    const int lane = threadIdx.x;
    const int bx = __builtin_amdgcn_readfirstlane(blockIdx.x), by = __builtin_amdgcn_readfirstlane(blockIdx.y);
    const int nx = a.nx, ny = a.ny, c = a.c, K = a.K;
    const long rs = a.rs, gs = a.gs, ss = a.ss;
    const int k = bx / pieces, m = bx - k * pieces;           // chunk k (with the separator east of it), its m-th piece of 128 columns
    const int scol = k < K ? k * c + c - 1 : -1;              // the separator column
    const int cend = k < K ? k * c + c : nx;                  // one past the last column of the chunk and its separator
    const int col = k * c + 128 * m + 2 * lane;               // an aligned pair: interior column 0 lies on a 16-byte boundary, c is even
    const bool ok0 = col < cend, ok1 = col + 1 < cend;
    const int r0 = by * XC_ROWS, r1 = min(r0 + XC_ROWS, ny);
    if (!ok0) return;
    const double *pt = a.t + col, *pu = a.u + col, *pv = a.t0 + col, *pw = a.t1 + col;
    double *po = a.out + col;
    const CDBL4 *xi = (const CDBL4 *)a.sep + 3L * K * ss;     // XI: read-only here, at wave-uniform addresses
    const double sc = a.scale;
    const bool issep = col + 1 == scol;                       // (the separator is an odd column: the second of its pair)
    auto pair = [&](const double *p) { return ok1 ? *reinterpret_cast<const double2 *>(p) : make_double2(*p, 0.0); };
    double2 v0 = make_double2(0.0, 0.0), w0 = make_double2(0.0, 0.0);
    if (gs == 0) {                                            // one table row for every grid row: loaded once
        if (k > 0) v0 = pair(pv);
        if (k < K) w0 = pair(pw);
    }
    for (int i0 = r0; i0 < r1; i0 += XC_R) {
        double2 rx[XC_R], ru[XC_R], rv[XC_R], rw[XC_R];
#pragma unroll
        for (int q = 0; q < XC_R; q++) {
            const long i = min(i0 + q, r1 - 1);
            rx[q] = pair(pt + i * rs);
            ru[q] = ZERO ? make_double2(0.0, 0.0) : pair(pu + i * rs);
            rv[q] = (gs != 0 && k > 0) ? pair(pv + i * gs) : v0;
            rw[q] = (gs != 0 && k < K) ? pair(pw + i * gs) : w0;
        }
#pragma unroll
        for (int q = 0; q < XC_R; q++) {
            const int i = i0 + q;
            if (i < r1) {                                     // (wave-uniform)
                double2 x = rx[q];
                double xhi = 0.0;
                if (k > 0) {
                    const double xlo = xi[(long)(k - 1) * ss + i];
                    const double p0 = xlo * rv[q].x, p1 = xlo * rv[q].y;
                    x.x = x.x - p0; x.y = x.y - p1;
                }
                if (k < K) {
                    xhi = xi[(long)k * ss + i];
                    const double p0 = xhi * rw[q].x, p1 = xhi * rw[q].y;
                    x.x = x.x - p0; x.y = x.y - p1;
                }
                x.y = issep ? xhi : x.y;                      // x_s = xi_k
                double2 o = make_double2(sc * x.x, sc * x.y);
                if (!ZERO) { o.x = ru[q].x + o.x; o.y = ru[q].y + o.y; }
                double *d = po + (long)i * rs;
                if (ok1) {
                    if (NT) st2_stream(d, o); else *reinterpret_cast<double2 *>(d) = o;
                } else if (NT) __builtin_nontemporal_store(o.x, d);
                else *d = o.x;
            }
        }
    }
}

template <bool ZERO>
__global__ void __launch_bounds__(64) k_xline_chunk_forward(const XChunkArgs a) {
    __shared__ double lds[4 * XTILE];
    if (line_store_nt(a.nt, a.ny, a.rs)) xchunk_forward_body<ZERO, true>(a, lds); else xchunk_forward_body<ZERO, false>(a, lds);
}
__global__ void __launch_bounds__(64) k_xline_chunk_backward(const XChunkArgs a) {
    __shared__ double lds[3 * XTILE];
    if (line_store_nt(a.nt, a.ny, a.rs)) xchunk_backward_body<true>(a, lds); else xchunk_backward_body<false>(a, lds);
}
__global__ void __launch_bounds__(64) k_xline_chunk_reduce(const XChunkArgs a) { xchunk_reduce_body(a); }
template <bool ZERO>
__global__ void __launch_bounds__(64) k_xline_chunk_correct(const XChunkArgs a, const int pieces) {
    if (line_store_nt(a.nt, a.ny, a.rs)) xchunk_correct_body<ZERO, true>(a, pieces); else xchunk_correct_body<ZERO, false>(a, pieces);
}

// 2-D, a period that is a positive multiple of the tile, no more chunks than a grid has rows, strides a window can address
bool xchunk_geom_ok(const mgk_geom *g, int c, long stride) {
    return line_geom_ok(g) && c > 0 && c % XT == 0 && g->nx / c + 1 <= 65535 && stride >= 0 && stride <= LINE_MAX_PITCH;
}
XChunkArgs xchunk_args(const mgk_geom *g, int c) {
    XChunkArgs a; memset(&a, 0, sizeof(a));
    a.nx = g->nx; a.ny = g->ny; a.c = c; a.K = g->nx / c; a.rs = g->pitch; a.ss = round16((long)g->ny); a.nt = store_policy();
    return a;
}
// the chunks a march is launched for: the last one only if it is not empty
unsigned xchunk_count(const XChunkArgs &a) { return (unsigned)(a.K + (a.nx > a.K * a.c ? 1 : 0)); }

}  // namespace

MGK_PRELOAD_UNIT(k_xline_chunk_backward)

extern "C" int mgk_xline_chunk_forward_f64(mgk_ctx *ctx, const mgk_geom *g, int c, const double *atab, const double *gtab, long gstride,
                                           const double *b, const double *u, double *t, double *sep, void *stream) {
    if (!ctx || !xchunk_geom_ok(g, c, gstride) || (gstride != 0 && gstride < g->nx) || !atab || !gtab || !b || !t || t == b || t == u || t == sep ||
        (g->nx >= c && !sep))
        return fail(MGK_EINVAL, "mgk_xline_chunk_forward_f64: bad arguments (2-D; c a positive multiple of 16; t must not alias b, u or sep; gstride 0 or >= nx)");
    XChunkArgs a = xchunk_args(g, c);
    a.u = u ? u + g->org : nullptr; a.b = b + g->org; a.t = t + g->org; a.sep = sep;
    a.ct = atab; a.t0 = gtab; a.gs = gstride;
    const dim3 grid((unsigned)((g->ny + 61) / 62), xchunk_count(a));
    if (u) hipLaunchKernelGGL(k_xline_chunk_forward<false>, grid, dim3(64), 0, S(ctx, stream), a);
    else hipLaunchKernelGGL(k_xline_chunk_forward<true>, grid, dim3(64), 0, S(ctx, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mgk_xline_chunk_backward_f64(mgk_ctx *ctx, const mgk_geom *g, int c, const double *atab, const double *gtab, long gstride,
                                            double *t, double *sep, void *stream) {
    if (!ctx || !xchunk_geom_ok(g, c, gstride) || (gstride != 0 && gstride < g->nx) || !atab || !gtab || !t || t == sep || (g->nx >= c && !sep))
        return fail(MGK_EINVAL, "mgk_xline_chunk_backward_f64: bad arguments (2-D; c a positive multiple of 16; t must not alias sep; gstride 0 or >= nx)");
    XChunkArgs a = xchunk_args(g, c);
    a.t = t + g->org; a.sep = sep; a.ct = atab; a.t0 = gtab; a.gs = gstride;
    const dim3 grid((unsigned)((g->ny + 63) / 64), xchunk_count(a));
    hipLaunchKernelGGL(k_xline_chunk_backward, grid, dim3(64), 0, S(ctx, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mgk_xline_chunk_reduce_f64(mgk_ctx *ctx, const mgk_geom *g, int c, const double *atab, const double *SLtab, const double *SGtab,
                                          const double *SQtab, long sstride, double *sep, void *stream) {
    if (!ctx || !xchunk_geom_ok(g, c, sstride) || (sstride != 0 && sstride < g->ny) || (g->nx >= c && (!atab || !SLtab || !SGtab || !SQtab || !sep)))
        return fail(MGK_EINVAL, "mgk_xline_chunk_reduce_f64: bad arguments (2-D; c a positive multiple of 16; sstride 0 or >= ny)");
    XChunkArgs a = xchunk_args(g, c);
    if (a.K == 0) return 0;                                   // no separator: nothing to solve
    a.sep = sep; a.ct = atab; a.t0 = SLtab; a.t1 = SGtab; a.t2 = SQtab; a.gs = sstride;
    const dim3 grid((unsigned)((g->ny + 63) / 64));
    hipLaunchKernelGGL(k_xline_chunk_reduce, grid, dim3(64), 0, S(ctx, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mgk_xline_chunk_correct_f64(mgk_ctx *ctx, const mgk_geom *g, int c, const double *vtab, const double *wtab, long gstride,
                                           double scale, const double *t, const double *sep, const double *u, double *unew, void *stream) {
    if (!ctx || !xchunk_geom_ok(g, c, gstride) || (gstride != 0 && gstride < g->nx) || (gstride & 1) || !t || !unew || unew == t || t == sep ||
        (g->nx >= c && (!vtab || !wtab || !sep || ((uintptr_t)vtab & 15) || ((uintptr_t)wtab & 15))))
        return fail(MGK_EINVAL, "mgk_xline_chunk_correct_f64: bad arguments (2-D; c a positive multiple of 16; unew must not alias t; gstride 0 or even and >= nx; "
                                "vtab, wtab 16-byte aligned)");
    XChunkArgs a = xchunk_args(g, c);
    a.t = const_cast<double *>(t) + g->org; a.sep = const_cast<double *>(sep); a.u = u ? u + g->org : nullptr; a.out = unew + g->org;
    a.t0 = vtab; a.t1 = wtab; a.gs = gstride; a.scale = scale;
    const int span = a.K ? c : g->nx, pieces = (span + 127) / 128;       // K = 0: the one chunk is the whole row
    const long rows = ((long)g->ny + XC_ROWS - 1) / XC_ROWS;
    if (rows > 65535) return fail(MGK_EINVAL, "mgk_xline_chunk_correct_f64: too many rows for one launch");
    const dim3 grid((unsigned)((long)(a.K + 1) * pieces), (unsigned)rows);
    if (u) hipLaunchKernelGGL(k_xline_chunk_correct<false>, grid, dim3(64), 0, S(ctx, stream), a, pieces);
    else hipLaunchKernelGGL(k_xline_chunk_correct<true>, grid, dim3(64), 0, S(ctx, stream), a, pieces);
    HIPCHK(hipGetLastError());
    return 0;
}
