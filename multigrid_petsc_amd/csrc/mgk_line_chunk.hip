// mgk_line_chunk.hip -- the y-line sweep of mgk_line.hip with its tridiagonal systems solved in chunks (the definition
// and the tables: include/mgk.h, csrc/mg_line_chunk.c): period c, K = ny / c, row s_j = j c + c - 1 is separator j, the rows
// [k c, min(k c + c - 1, ny)) are chunk k.  The Thomas recurrence is serial along y and a lane owns a column, so the plain passes run on
// nx / 62 waves whatever the height; here every chunk is a wave of its own, (K + 1) times as many.  Four passes over one scratch field t:
//   mgk_line_chunk_forward_f64    one wave per (62-column tile, chunk): the residual (x neighbours by DPP wave shifts, as k_line_forward), the
//                                 forward substitution restarted at the chunk's first row, t = y g; the separator below the chunk gets its r_s
//   mgk_line_chunk_backward_f64   one wave per (64-column tile, chunk): the back substitution, t -> x' in place (a point reads only itself)
//   mgk_line_chunk_reduce_f64     a lane owns a column and marches over the K separators: rho_j from the three rows around s_j, down (Z_j kept
//                                 in row s_j), then up (xi_j over it); the loads of the next four separators are issued ahead of the four in hand
//   mgk_line_chunk_correct_f64    streaming: a lane owns an aligned column pair (16-byte accesses), a wave 128 columns of up to 16 rows of ONE
//                                 chunk, so that xi of the two separators around it is loaded once; x = (x' - xi_{k-1} v) - xi_k w, u' = u + s x
// fp64, no FMA (-ffp-contract=off).  Every wave is a block of its own; the chunk and the tile come from blockIdx through readfirstlane, so the
// row arithmetic is scalar, and the per-row tables are read through the constant address space at wave-uniform addresses: scalar loads
// (DESIGN.md section 4 (xviii)).  The marches issue the loads of CH_R rows before they use the first.  Nothing outside the interior of an
// output is written; loads touch the ghost ring at most.  Stores: mgk_store_nt_2d, or the policy mgk_set_tuning(0 / 1) forces.
#include "mgk_line_dev.hpp"

namespace {

struct ChunkArgs {
    const double *u, *b;            // forward: u (unused from the zero guess), b; correct: u (unused from the zero guess)
    double *t;                      // the scratch field: forward writes it, backward and reduce update it in place, correct reads it
    double *out;                    // correct: unew
    const double *t0, *t1, *t2, *t3;   // forward: row table (ny x 5), ltab, gtab; backward: qtab; reduce: row table, L, G, Q; correct: vtab, wtab
    int nx, ny, c, K;
    long rs;
    double scale;
    int nt;                         // store policy: < 0 by size, 0 ordinary, 1 non-temporal
};

constexpr int CH_R = 8;             // rows (reduce: separators, CH_S) whose loads are in flight together
constexpr int CH_S = 4;
constexpr int CH_ROWS = 16;         // rows of a wave of the correction pass

template <bool NT> __device__ __forceinline__ void chunk_st(double *p, double v) {
    if (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

template <bool ZERO, bool NT>
__device__ __forceinline__ void chunk_forward_body(const ChunkArgs &a) {
    const int lane = threadIdx.x;
    const int tx = __builtin_amdgcn_readfirstlane(blockIdx.x), k = __builtin_amdgcn_readfirstlane(blockIdx.y);
    const int nx = a.nx, ny = a.ny, c = a.c;
    const long rs = a.rs;
    const int r0 = k * c;                                     // the chunk's first row
    const int sep = k < a.K ? r0 + c - 1 : -1;                // the separator below it (<= ny - 1), whose residual this wave stores as well
    const int r1 = k < a.K ? r0 + c : ny;                     // one past the last row this wave writes
    if (r0 >= r1) return;                                     // ny = K c: the last chunk is empty
    const int cb = tx * 62 - 1;                               // column of lane 0; -1 and nx are the ghost columns (zero)
    const bool store = lane >= 1 && lane <= 62 && cb + lane < nx;
    const long col = min(cb + lane, nx);                      // loads: every lane in range (columns clamped to the ghost column nx)
    const double *pb = a.b + col, *pu = a.u + col;
    double *pz = a.t + col;
    const CDBL4 *ct = (const CDBL4 *)a.t0, *lt = (const CDBL4 *)a.t1, *gt = (const CDBL4 *)a.t2;
    double ua = 0.0, ub = 0.0;                                // u of the rows i - 1 (row -1: ghost) and i
    if (!ZERO) {
        ua = pu[(long)(r0 - 1) * rs];
        ub = pu[(long)r0 * rs];
    }
    double y = 0.0;
    for (int i0 = r0; i0 < r1; i0 += CH_R) {
        double rb[CH_R], ru[CH_R];
#pragma unroll
        for (int q = 0; q < CH_R; q++) {                      // rows past the last one: clamped loads, nothing computed
            const int i = min(i0 + q, r1 - 1);
            rb[q] = pb[(long)i * rs];
            ru[q] = ZERO ? 0.0 : pu[(long)(i + 1) * rs];      // row ny: the ghost row
        }
#pragma unroll
        for (int q = 0; q < CH_R; q++) {
            const int i = i0 + q;
            if (i < r1) {                                     // (wave-uniform)
                double r = rb[q];
                if (!ZERO) {
                    const double uc = ru[q];
                    const double wv = lane_up<true>(ub), ev = lane_dn<true>(ub);
                    const CDBL4 *cr = ct + 5 * (long)i;
                    double t = cr[0] * ua;
                    t = t + cr[1] * wv;
                    t = t + cr[2] * ub;
                    t = t + cr[3] * ev;
                    t = t + cr[4] * uc;
                    r = r - t;
                    ua = ub; ub = uc;
                }
                double zz = r;                                // the separator row keeps its residual
                if (i != sep) {
                    if (i == r0) y = r;
                    else {
                        const double ly = lt[i] * y;
                        y = r - ly;
                    }
                    zz = y * gt[i];
                }
                if (store) chunk_st<NT>(pz + (long)i * rs, zz);
            }
        }
    }
}

template <bool NT>
__device__ __forceinline__ void chunk_backward_body(const ChunkArgs &a) {
    const int lane = threadIdx.x;
    const int tx = __builtin_amdgcn_readfirstlane(blockIdx.x), k = __builtin_amdgcn_readfirstlane(blockIdx.y);
    const int nx = a.nx, ny = a.ny, c = a.c;
    const long rs = a.rs;
    const int r0 = k * c, r1 = k < a.K ? r0 + c - 1 : ny;     // the chunk: rows [r0, r1)
    if (r0 >= r1) return;
    const int cb = tx * 64;
    const bool store = cb + lane < nx;
    double *p = a.t + min(cb + lane, nx);
    const CDBL4 *qt = (const CDBL4 *)a.t0;
    double e = 0.0;
    for (int i0 = r1 - 1; i0 >= r0; i0 -= CH_R) {
        double rz[CH_R];
#pragma unroll
        for (int q = 0; q < CH_R; q++) rz[q] = p[(long)max(i0 - q, r0) * rs];
#pragma unroll
        for (int q = 0; q < CH_R; q++) {
            const int i = i0 - q;
            if (i >= r0) {                                    // (wave-uniform)
                if (i == r1 - 1) e = rz[q];                   // x'_{b-1} = z_{b-1}: already in place
                else {
                    const double qe = qt[i] * e;
                    e = rz[q] - qe;
                    if (store) chunk_st<NT>(p + (long)i * rs, e);
                }
            }
        }
    }
}

template <bool NT>
__device__ __forceinline__ void chunk_reduce_body(const ChunkArgs &a) {
    const int lane = threadIdx.x;
    const int tx = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int nx = a.nx, ny = a.ny, c = a.c, K = a.K;
    const long rs = a.rs;
    const int cb = tx * 64;
    const bool store = cb + lane < nx;
    double *p = a.t + min(cb + lane, nx);
    const CDBL4 *ct = (const CDBL4 *)a.t0, *Lt = (const CDBL4 *)a.t1, *Gt = (const CDBL4 *)a.t2, *Qt = (const CDBL4 *)a.t3;
    // both marches are software-pipelined: the loads of the NEXT CH_S separators are issued before the serial recurrence of the CH_S in
    // hand, so their latency lies behind it (a wave per 64 columns: occupancy hides nothing here).  The rows a batch stores (its own
    // separator rows) are read by no later batch of the same march.
    double Y = 0.0, Z = 0.0;
    double xm[CH_S], x0[CH_S], xp[CH_S], nm[CH_S], n0[CH_S], np[CH_S];
    auto load_down = [&](int j0, double *am, double *a0, double *ap) {
#pragma unroll
        for (int q = 0; q < CH_S; q++) {
            const long s = (long)min(j0 + q, K - 1) * c + c - 1;
            am[q] = p[(s - 1) * rs];
            a0[q] = p[s * rs];
            ap[q] = p[min(s + 1, (long)ny - 1) * rs];
        }
    };
    load_down(0, xm, x0, xp);
    for (int j0 = 0; j0 < K; j0 += CH_S) {                    // down: Z_j into row s_j
        load_down(j0 + CH_S, nm, n0, np);                     // (past the last separator: clamped, unused)
#pragma unroll
        for (int q = 0; q < CH_S; q++) {
            const int j = j0 + q;
            if (j < K) {                                      // (wave-uniform)
                const long s = (long)j * c + c - 1;
                const CDBL4 *cr = ct + 5 * s;
                double t = cr[0] * xm[q];
                double rho = x0[q] - t;
                if (s < ny - 1) {
                    t = cr[4] * xp[q];
                    rho = rho - t;
                }
                if (j == 0) Y = rho;
                else {
                    t = Lt[j] * Y;
                    Y = rho - t;
                }
                Z = Y * Gt[j];
                if (store) chunk_st<NT>(p + s * rs, Z);
            }
        }
#pragma unroll
        for (int q = 0; q < CH_S; q++) { xm[q] = nm[q]; x0[q] = n0[q]; xp[q] = np[q]; }
    }
    double xi = Z;                                            // xi_{K-1} = Z_{K-1}: already in place
    auto load_up = [&](int j0, double *a) {
#pragma unroll
        for (int q = 0; q < CH_S; q++) a[q] = p[((long)max(j0 - q, 0) * c + c - 1) * rs];
    };
    load_up(K - 2, x0);
    for (int j0 = K - 2; j0 >= 0; j0 -= CH_S) {               // up: xi_j over Z_j (this lane's own stores of the march down)
        load_up(j0 - CH_S, n0);
#pragma unroll
        for (int q = 0; q < CH_S; q++) {
            const int j = j0 - q;
            if (j >= 0) {
                const double t = Qt[j] * xi;
                xi = x0[q] - t;
                if (store) chunk_st<NT>(p + ((long)j * c + c - 1) * rs, xi);
            }
        }
#pragma unroll
        for (int q = 0; q < CH_S; q++) x0[q] = n0[q];
    }
}

template <bool ZERO, bool NT>
__device__ __forceinline__ void chunk_correct_body(const ChunkArgs &a, int pieces) {
    const int lane = threadIdx.x;
    const int tx = __builtin_amdgcn_readfirstlane(blockIdx.x), by = __builtin_amdgcn_readfirstlane(blockIdx.y);
    const int nx = a.nx, ny = a.ny, c = a.c, K = a.K;
    const long rs = a.rs;
    const int k = by / pieces, m = by - k * pieces;           // chunk k (with the separator below it), its m-th piece of CH_ROWS rows
    const int r0 = k * c + m * CH_ROWS;
    const int r1 = min(min(r0 + CH_ROWS, k < K ? k * c + c : ny), ny);
    if (r0 >= r1) return;
    const int sep = k < K ? k * c + c - 1 : -1;
    const long col = 2L * (tx * 64 + lane);                   // an aligned pair: interior column 0 lies on a 16-byte boundary
    const bool ok0 = col < nx, ok1 = col + 1 < nx;            // (the column nx of a pair is the ghost column: read, never written)
    if (!ok0) return;
    const double *pt = a.t + col, *pu = a.u + col;
    double *po = a.out + col;
    const CDBL4 *vt = (const CDBL4 *)a.t0, *wt = (const CDBL4 *)a.t1;
    const double sc = a.scale;
    double2 xlo = make_double2(0.0, 0.0), xhi = make_double2(0.0, 0.0);       // xi of the separators above and below the chunk
    if (k > 0) xlo = *reinterpret_cast<const double2 *>(pt + (long)(k * c - 1) * rs);
    if (k < K) xhi = *reinterpret_cast<const double2 *>(pt + (long)sep * rs);
    for (int i0 = r0; i0 < r1; i0 += CH_R) {
        double2 rx[CH_R], ru[CH_R];
#pragma unroll
        for (int q = 0; q < CH_R; q++) {
            const long i = min(i0 + q, r1 - 1);
            rx[q] = *reinterpret_cast<const double2 *>(pt + i * rs);
            ru[q] = ZERO ? make_double2(0.0, 0.0) : *reinterpret_cast<const double2 *>(pu + i * rs);
        }
#pragma unroll
        for (int q = 0; q < CH_R; q++) {
            const int i = i0 + q;
            if (i < r1) {                                     // (wave-uniform)
                double2 x = rx[q];
                if (i != sep) {
                    if (k > 0) {
                        const double v = vt[i];
                        const double p0 = xlo.x * v, p1 = xlo.y * v;
                        x.x = x.x - p0; x.y = x.y - p1;
                    }
                    if (k < K) {
                        const double w = wt[i];
                        const double p0 = xhi.x * w, p1 = xhi.y * w;
                        x.x = x.x - p0; x.y = x.y - p1;
                    }
                }
                double2 o = make_double2(sc * x.x, sc * x.y);
                if (!ZERO) { o.x = ru[q].x + o.x; o.y = ru[q].y + o.y; }
                double *d = po + (long)i * rs;
                if (ok1) {
                    if (NT) st2_stream(d, o); else *reinterpret_cast<double2 *>(d) = o;
                } else chunk_st<NT>(d, o.x);
            }
        }
    }
}

template <bool ZERO>
__global__ void __launch_bounds__(64) k_line_chunk_forward(const ChunkArgs a) {
    if (line_store_nt(a.nt, a.ny, a.rs)) chunk_forward_body<ZERO, true>(a); else chunk_forward_body<ZERO, false>(a);
}
__global__ void __launch_bounds__(64) k_line_chunk_backward(const ChunkArgs a) {
    if (line_store_nt(a.nt, a.ny, a.rs)) chunk_backward_body<true>(a); else chunk_backward_body<false>(a);
}
__global__ void __launch_bounds__(64) k_line_chunk_reduce(const ChunkArgs a) {
    if (line_store_nt(a.nt, a.ny, a.rs)) chunk_reduce_body<true>(a); else chunk_reduce_body<false>(a);
}
template <bool ZERO>
__global__ void __launch_bounds__(64) k_line_chunk_correct(const ChunkArgs a, const int pieces) {
    if (line_store_nt(a.nt, a.ny, a.rs)) chunk_correct_body<ZERO, true>(a, pieces); else chunk_correct_body<ZERO, false>(a, pieces);
}

// 2-D, a period of at least two rows, and no more chunks than a grid has rows
bool chunk_geom_ok(const mgk_geom *g, int c) {
    return line_dims_ok(g) && c >= 2 && g->ny / c + 1 <= 65535;
}
ChunkArgs chunk_args(const mgk_geom *g, int c) {
    ChunkArgs a; memset(&a, 0, sizeof(a));
    a.nx = g->nx; a.ny = g->ny; a.c = c; a.K = g->ny / c; a.rs = g->pitch; a.nt = store_policy();
    return a;
}

}  // namespace

MGK_PRELOAD_UNIT(k_line_chunk_backward)

extern "C" int mgk_line_chunk_forward_f64(mgk_ctx *ctx, const mgk_geom *g, int c, const double *atab, const double *ltab, const double *gtab,
                                          const double *b, const double *u, double *t, void *stream) {
    if (!ctx || !chunk_geom_ok(g, c) || !ltab || !gtab || !b || !t || (u && !atab) || t == b || t == u)
        return fail(MGK_EINVAL, "mgk_line_chunk_forward_f64: bad arguments (2-D; c >= 2; t must not alias b or u)");
    ChunkArgs a = chunk_args(g, c);
    a.u = u ? u + g->org : nullptr; a.b = b + g->org; a.t = t + g->org;
    a.t0 = atab; a.t1 = ltab; a.t2 = gtab;
    const dim3 grid((unsigned)((g->nx + 61) / 62), (unsigned)(a.K + (g->ny > a.K * c ? 1 : 0)));
    if (u) hipLaunchKernelGGL(k_line_chunk_forward<false>, grid, dim3(64), 0, S(ctx, stream), a);
    else hipLaunchKernelGGL(k_line_chunk_forward<true>, grid, dim3(64), 0, S(ctx, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mgk_line_chunk_backward_f64(mgk_ctx *ctx, const mgk_geom *g, int c, const double *qtab, double *t, void *stream) {
    if (!ctx || !chunk_geom_ok(g, c) || !qtab || !t)
        return fail(MGK_EINVAL, "mgk_line_chunk_backward_f64: bad arguments (2-D; c >= 2)");
    ChunkArgs a = chunk_args(g, c);
    a.t = t + g->org; a.t0 = qtab;
    const dim3 grid((unsigned)((g->nx + 63) / 64), (unsigned)(a.K + (g->ny > a.K * c ? 1 : 0)));
    hipLaunchKernelGGL(k_line_chunk_backward, grid, dim3(64), 0, S(ctx, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mgk_line_chunk_reduce_f64(mgk_ctx *ctx, const mgk_geom *g, int c, const double *atab, const double *Ltab, const double *Gtab,
                                         const double *Qtab, double *t, void *stream) {
    if (!ctx || !chunk_geom_ok(g, c) || !t || (g->ny >= c && (!atab || !Ltab || !Gtab || !Qtab)))
        return fail(MGK_EINVAL, "mgk_line_chunk_reduce_f64: bad arguments (2-D; c >= 2)");
    ChunkArgs a = chunk_args(g, c);
    if (a.K == 0) return 0;                                   // no separator: nothing to solve
    a.t = t + g->org; a.t0 = atab; a.t1 = Ltab; a.t2 = Gtab; a.t3 = Qtab;
    const dim3 grid((unsigned)((g->nx + 63) / 64));
    hipLaunchKernelGGL(k_line_chunk_reduce, grid, dim3(64), 0, S(ctx, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mgk_line_chunk_correct_f64(mgk_ctx *ctx, const mgk_geom *g, int c, const double *vtab, const double *wtab, double scale,
                                          const double *t, const double *u, double *unew, void *stream) {
    if (!ctx || !chunk_geom_ok(g, c) || !t || !unew || unew == t || (g->ny >= c && (!vtab || !wtab)))
        return fail(MGK_EINVAL, "mgk_line_chunk_correct_f64: bad arguments (2-D; c >= 2; unew must not alias t)");
    ChunkArgs a = chunk_args(g, c);
    a.t = const_cast<double *>(t) + g->org; a.u = u ? u + g->org : nullptr; a.out = unew + g->org;
    a.t0 = vtab; a.t1 = wtab; a.scale = scale;
    const int span = a.K ? c : g->ny, pieces = (span + CH_ROWS - 1) / CH_ROWS;      // K = 0: the one chunk is the whole column
    const long rows = (long)(a.K + 1) * pieces;
    if (rows > 65535) return fail(MGK_EINVAL, "mgk_line_chunk_correct_f64: too many chunks for one launch");
    const dim3 grid((unsigned)((g->nx + 127) / 128), (unsigned)rows);
    if (u) hipLaunchKernelGGL(k_line_chunk_correct<false>, grid, dim3(64), 0, S(ctx, stream), a, pieces);
    else hipLaunchKernelGGL(k_line_chunk_correct<true>, grid, dim3(64), 0, S(ctx, stream), a, pieces);
    HIPCHK(hipGetLastError());
    return 0;
}
