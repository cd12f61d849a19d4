// mgk_line.hip -- y-line Jacobi on the 2-D row-table operators: one sweep u <- u + s T^-1 (b - A u), T = the
// y-tridiagonal part of A.  The coefficients depend on the grid row only, so every column has the SAME tridiagonal matrix and its
// factorisation is three more per-row tables made on the host (mg_line.c): l (the multipliers), g (1 / pivot), q = N g.
//   mgk_line_forward_f64    r_i = b_i - (A u)_i (five terms in the order of mgk_rowcoef_f64 mode 1; from the zero guess r = b, u is not read)
//                           y_0 = r_0, y_i = r_i - l_i y_{i-1};  z_i = y_i g_i, stored                  24 B per unknown (zero guess: 16)
//   mgk_line_backward_f64   e_{n-1} = z_{n-1}, e_i = z_i - q_i e_{i+1};  u'_i = u_i + s e_i (zero guess: s e_i)   24 B per unknown (16)
// fp64, no FMA (-ffp-contract=off); one multiply and one subtract per row on the dependent chain, the products with g off it.
// Every WAVE is independent (no LDS, no barrier) and is a block of its own, so that the few waves a level has (67 forward, 64 backward at
// 4095^2) spread over the CUs.  A lane owns ONE column and marches over ALL rows: down in the forward pass, up in the backward pass.
// Forward: lane l of wave tx holds column 62 tx + l - 1, the x neighbours of u come by DPP wave shifts, lanes 1 .. 62 store (tiles overlap
// by two lanes).  Backward: a point reads only itself, 64 columns per wave.  The loads of u, b and z are issued D rows ahead through a
// statically indexed register ring; the loop is unrolled by a period of 32 rows that is one basic block (see the bodies).  Loads and
// stores go through buffer descriptors: a row is a scalar byte offset, the column a constant VGPR, and a lane that must not store has
// a lane offset out of range, which the hardware drops -- no branch, no 64-bit vector address arithmetic.  Loads are unconditional, their
// row indices clamped on the scalar unit.  The row tables come in chunks of 16 rows through the vector unit and are handed out by DPP
// row broadcasts (scalar loads return out of order: a load per row would expose its latency in every row).  The ghost ring of no field
// is written, and the backward pass may write u in place: a sweep swaps no buffers.
// Stores: every pass reads what the one before it wrote, so fields within the 256 MB Infinity Cache are stored
// normally and only larger ones non-temporally (mgk_store_nt_2d); mgk_set_tuning(variant = 0 / 1) forces one policy, and its second
// argument (> 0) the prefetch depth (rounded down to a built one: 8, 16, 32).
#include "mgk_line_dev.hpp"

namespace {

struct LineArgs {
    const double *u, *b, *z;        // forward: u (unused from the zero guess), b; backward: z, u (unused from the zero guess)
    double *out;                    // forward: z; backward: unew
    const double *t0, *t1, *t2;     // forward: the row table (ny x 5), ltab, gtab; backward: qtab
    int nx, ny;
    long rs;
    double scale;
    int nt;                         // store policy: < 0 by size, 0 ordinary, 1 non-temporal
};

constexpr int LINE_U = 32;                      // rows per unrolled period: two table chunks of 16 rows, a multiple of every ring depth
static_assert((LINE_U + 32 + 3) * LINE_MAX_PITCH * 8 < (1L << 31), "the rows of a window: a period, the deepest ring, the rows around them");

// lane K of every row of 16 lanes, to all lanes of that row (DPP row_newbcast): a table value that lane K of each row loaded
template <int K> __device__ __forceinline__ double line_bcast(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x150 + K, 0xf, 0xf, true);      // every lane has a source: no old value to keep
    hi = __builtin_amdgcn_mov_dpp(hi, 0x150 + K, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// Both bodies: a period of LINE_U rows is ONE basic block.  Row i consumes ring slot i mod D and only then reloads it for row i + D; a
// scheduling barrier after every row keeps that order, so the ring stays in its registers and the wait before a row leaves the loads and
// stores of the D - 1 rows after it in flight.  Rows past the last one (the last, CHECKED period) compute on clamped loads and store
// nothing.  The row tables come in chunks of 16 rows, one chunk ahead: lane t of every row of 16 lanes loads table row (chunk + t).
template <int D, bool ZERO, bool NT>
__device__ __forceinline__ void line_forward_body(const LineArgs &a) {
    static_assert(LINE_U % D == 0 && LINE_U % 32 == 0 && D <= 32, "ring depth");
    const int lane = threadIdx.x;
    const int tx = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int cb = tx * 62 - 1;                               // column of lane 0; -1 and nx are the ghost columns (zero)
    const int nx = a.nx, ny = a.ny;
    const long rs = a.rs;
    const bool store = lane >= 1 && lane <= 62 && cb + lane < nx;
    const unsigned vo = (unsigned)min(lane, nx - cb) * 8u;    // loads: every lane in range (columns clamped to the ghost column nx)
    const unsigned vs = store ? vo : LINE_OOB;
    const unsigned rb8 = (unsigned)rs * 8u;
    const int t16 = lane & 15;
    double rb[D], ru[D];                                      // ring slot k: b of row i, u of row i + 1 for i = k (mod D)
    double tc[2][5], tl[2], tg[2];                            // table chunks: lane t of a row of 16 holds table row (chunk + t)
    auto load_tab = [&](int set, int r0) {
        const long ri = min(r0 + t16, ny - 1);
        if (!ZERO) {
#pragma unroll
            for (int j = 0; j < 5; j++) tc[set][j] = a.t0[5 * ri + j];
        }
        tl[set] = a.t1[ri];
        tg[set] = a.t2[ri];
    };
    // the prologue in the order of age the steady state has: tables, the rows in hand, the ring
    load_tab(0, 0);
    double ua = 0.0, ub = 0.0;                                // rows i - 1 (row -1: ghost) and i
    {
        const __amdgpu_buffer_rsrc_t wu = line_window(a.u, cb, -1, rs), wb = line_window(a.b, cb, -1, rs);
        if (!ZERO) {
            ua = line_ld(wu, vo, 0);
            ub = line_ld(wu, vo, rb8);
        }
#pragma unroll
        for (int k = 0; k < D; k++) {
            rb[k] = line_ld(wb, vo, (unsigned)(min(k, ny - 1) + 1) * rb8);
            ru[k] = ZERO ? 0.0 : line_ld(wu, vo, (unsigned)(min(k + 1, ny) + 1) * rb8);
        }
    }
    double y = 0.0;
    auto period = [&](int i0, auto checked) {
        constexpr bool CHECKED = decltype(checked)::value;
        const __amdgpu_buffer_rsrc_t wu = line_window(a.u, cb, i0 - 1, rs), wb = line_window(a.b, cb, i0 - 1, rs),
                                     wz = line_window(a.out, cb, i0 - 1, rs);
        LineUnroll<0, LINE_U>::run([&](auto kc) {
            constexpr int k = decltype(kc)::value, s = k % D, ts = (k / 16) & 1, tk = k % 16;
            if (tk == 0) load_tab(ts ^ 1, i0 + k + 16);
            const double bi = rb[s];
            double r = bi;
            if (!ZERO) {
                const double uc = ru[s];
                const double wv = lane_up<true>(ub), ev = lane_dn<true>(ub);
                double t = line_bcast<tk>(tc[ts][0]) * ua;
                t = t + line_bcast<tk>(tc[ts][1]) * wv;
                t = t + line_bcast<tk>(tc[ts][2]) * ub;
                t = t + line_bcast<tk>(tc[ts][3]) * ev;
                t = t + line_bcast<tk>(tc[ts][4]) * uc;
                r = bi - t;
                ua = ub; ub = uc;
            }
            const double ly = line_bcast<tk>(tl[ts]) * y;
            y = r - ly;
            const double zz = y * line_bcast<tk>(tg[ts]);
            line_st<NT>(zz, wz, CHECKED ? (i0 + k < ny ? vs : LINE_OOB) : vs, (unsigned)(k + 1) * rb8);
            rb[s] = line_ld(wb, vo, (unsigned)(min(i0 + k + D, ny - 1) - i0 + 1) * rb8);
            if (!ZERO) ru[s] = line_ld(wu, vo, (unsigned)(min(i0 + k + 1 + D, ny) - i0 + 1) * rb8);
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    int i0 = 0;
    for (; i0 + LINE_U <= ny; i0 += LINE_U) period(i0, std::false_type{});
    if (i0 < ny) period(i0, std::true_type{});
}

template <int D, bool ZERO, bool NT>
__device__ __forceinline__ void line_backward_body(const LineArgs &a) {
    static_assert(LINE_U % D == 0 && LINE_U % 32 == 0 && D <= 32, "ring depth");
    const int lane = threadIdx.x;
    const int tx = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const int cb = tx * 64;
    const int nx = a.nx, ny = a.ny;
    const long rs = a.rs;
    const bool store = cb + lane < nx;
    const unsigned vo = (unsigned)min(lane, nx - cb) * 8u;
    const unsigned vs = store ? vo : LINE_OOB;
    const unsigned rb8 = (unsigned)rs * 8u;
    const int t16 = lane & 15;
    const double sc = a.scale;
    double rz[D], ru[D];                                      // ring slot k: z and u of row i = ny - 1 - j, j = k (mod D)
    double tq[2];
    auto load_tab = [&](int set, int j0) { tq[set] = a.t0[max(ny - 1 - j0 - t16, 0)]; };
    load_tab(0, 0);
    {
        const int bw = ny - 1 - D;                            // window base row (may lie before the field; rows are clamped to >= 0)
        const __amdgpu_buffer_rsrc_t wz = line_window(a.z, cb, bw, rs), wu = line_window(a.u, cb, bw, rs);
#pragma unroll
        for (int k = 0; k < D; k++) {
            const unsigned o = (unsigned)(max(ny - 1 - k, 0) - bw) * rb8;
            rz[k] = line_ld(wz, vo, o);
            ru[k] = ZERO ? 0.0 : line_ld(wu, vo, o);
        }
    }
    double e = 0.0;
    auto period = [&](int j0, auto checked) {
        constexpr bool CHECKED = decltype(checked)::value;
        const int hi = ny - 1 - j0, bw = hi - (LINE_U + D);   // rows hi, hi - 1, ...; reloads reach down to hi - (LINE_U - 1) - D
        const __amdgpu_buffer_rsrc_t wz = line_window(a.z, cb, bw, rs), wu = line_window(a.u, cb, bw, rs), wo = line_window(a.out, cb, bw, rs);
        LineUnroll<0, LINE_U>::run([&](auto kc) {
            constexpr int k = decltype(kc)::value, s = k % D, ts = (k / 16) & 1, tk = k % 16;
            if (tk == 0) load_tab(ts ^ 1, j0 + k + 16);
            const double zi = rz[s];
            const double qe = line_bcast<tk>(tq[ts]) * e;
            e = zi - qe;
            const double se = sc * e;
            double o = se;
            if (!ZERO) o = ru[s] + se;
            line_st<NT>(o, wo, CHECKED ? (j0 + k < ny ? vs : LINE_OOB) : vs, (unsigned)(LINE_U + D - k) * rb8);
            const unsigned on = (unsigned)(max(hi - k - D, 0) - bw) * rb8;
            rz[s] = line_ld(wz, vo, on);
            if (!ZERO) ru[s] = line_ld(wu, vo, on);
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    int j0 = 0;
    for (; j0 + LINE_U <= ny; j0 += LINE_U) period(j0, std::false_type{});
    if (j0 < ny) period(j0, std::true_type{});
}

template <int D, bool ZERO>
__global__ void __launch_bounds__(64) k_line_forward(const LineArgs a) {
    if (line_store_nt(a.nt, a.ny, a.rs)) line_forward_body<D, ZERO, true>(a); else line_forward_body<D, ZERO, false>(a);
}
template <int D, bool ZERO>
__global__ void __launch_bounds__(64) k_line_backward(const LineArgs a) {
    if (line_store_nt(a.nt, a.ny, a.rs)) line_backward_body<D, ZERO, true>(a); else line_backward_body<D, ZERO, false>(a);
}

int line_depth() { return g_zchunk >= 32 ? 32 : g_zchunk >= 16 ? 16 : g_zchunk > 0 ? 8 : 16; }
// the built ring depths, as with_depth lists them: 8 and 32 by name, 16 for everything else
template <typename F> void line_depths(int d, F &&f) { with_depth<8, 32, 16>(d, f); }

}  // namespace

MGK_PRELOAD_UNIT(k_line_backward<16, false>)

extern "C" int mgk_line_forward_f64(mgk_ctx *c, const mgk_geom *g, const double *atab, const double *ltab, const double *gtab,
                                    const double *b, const double *u, double *z, void *stream) {
    if (!c || !line_geom_ok(g) || !ltab || !gtab || !b || !z || (u && !atab) || z == b || z == u)
        return fail(MGK_EINVAL, "mgk_line_forward_f64: bad arguments (2-D; z must not alias b or u)");
    LineArgs a; memset(&a, 0, sizeof(a));
    a.u = u ? u + g->org : nullptr; a.b = b + g->org; a.out = z + g->org;
    a.t0 = atab; a.t1 = ltab; a.t2 = gtab;
    a.nx = g->nx; a.ny = g->ny; a.rs = g->pitch; a.nt = store_policy();
    const dim3 grid((unsigned)((g->nx + 61) / 62));
    LAUNCH_DEPTH_ZERO(line_depths, line_depth(), u == nullptr, k_line_forward, grid, S(c, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mgk_line_backward_f64(mgk_ctx *c, const mgk_geom *g, const double *qtab, double scale, const double *z, const double *u,
                                     double *unew, void *stream) {
    if (!c || !line_geom_ok(g) || !qtab || !z || !unew || unew == z)
        return fail(MGK_EINVAL, "mgk_line_backward_f64: bad arguments (2-D; unew must not alias z)");
    LineArgs a; memset(&a, 0, sizeof(a));
    a.z = z + g->org; a.u = u ? u + g->org : nullptr; a.out = unew + g->org;
    a.t0 = qtab;
    a.nx = g->nx; a.ny = g->ny; a.rs = g->pitch; a.scale = scale; a.nt = store_policy();
    const dim3 grid((unsigned)((g->nx + 63) / 64));
    LAUNCH_DEPTH_ZERO(line_depths, line_depth(), u == nullptr, k_line_backward, grid, S(c, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}
