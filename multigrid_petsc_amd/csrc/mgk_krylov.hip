// mgk_krylov.hip -- the orthogonalisation of restarted GMRES (csrc/mg_gmres.c) on level fields: the passes of one Arnoldi step with j basis
// vectors, each reading its operands ONCE.
//   mgk_multi_dot_f64         out[i] = v_i . w, i < k, one pass over w and the k basis fields                (8k + 8) B per unknown
//   mgk_multi_axpy_sumsq_f64  w <- (..((w - h_0 v_0) - h_1 v_1)..) - h_{k-1} v_{k-1} and ||w_new||^2          (8k + 16) B per unknown
//   mgk_lincomb_f64           out = (..(y_0 v_0 + y_1 v_1)..) + y_{k-1} v_{k-1}   (the correction at a restart)
//   mgk_scale_to_f64          out [and out2] = a x                                 (v_{j+1} = w / ||w||)
// Written with mgk_flat_dot / mgk_flat_axpy a step would read w 2k times ((32k + 24) B per unknown) and cross to the host k times.
// Padded level layout (mgk_geom), fp64, no FMA (-ffp-contract=off), sums over interior points only, nothing outside the interior of
// an output is written.  Reductions: one partial per block and operand, finished in a fixed order by one block per value -- no
// floating-point atomics, the same bits on every run.  A lane owns two neighbouring columns and walks down its share of the rows; for every
// row it issues the 16-byte loads of all k operands before the first of them is used.
// Stores: every one of these passes reads what the launch before it wrote, so fields within the 256 MB Infinity
// Cache are stored normally and only larger ones non-temporally (mgk_store_nt_2d); mgk_set_tuning(variant = 0 / 1) forces one policy.
#include "mgk_dev.hpp"

namespace {

struct KryArgs {
    int nx, ny, npairs, k;
    long pitch, plane, nrows;       // nrows = ny * nz
    int nt;                         // store policy: < 0 by size, 0 ordinary, 1 non-temporal
    const double *v[MGK_KRYLOV_MAX];
};
struct KryCoefs { double y[MGK_KRYLOV_MAX]; };

__device__ __forceinline__ long kry_row_offset(const KryArgs &a, long row) {
    const long k = row / a.ny, i = row - k * a.ny;
    return k * a.plane + i * a.pitch;
}
__device__ __forceinline__ bool kry_nt(const KryArgs &a) { return a.nt < 0 ? mgk_store_nt_2d((int)(a.nrows > 0x7fffffffL ? 0x7fffffffL : a.nrows), a.pitch) : a.nt != 0; }
// the last pair of a row holds the right ghost column in its second half: that half is neither summed nor written
__device__ __forceinline__ void kry_store(double *p, double2 v, bool half, bool nt) {
    if (half) { *p = v.x; return; }
    V16<double> t; t.v[0] = v.x; t.v[1] = v.y;
    stv_policy(p, t, nt);
}
#define KRY_ROWS(a)                                                                          \
    const long rpb_ = ((a).nrows + gridDim.y - 1) / gridDim.y;                               \
    const long row0_ = (long)blockIdx.y * rpb_;                                              \
    const long row1_ = (row0_ + rpb_ < (a).nrows) ? row0_ + rpb_ : (a).nrows;                \
    for (long row = row0_; row < row1_; row++)

template <int KB>
__global__ void __launch_bounds__(256) k_multi_dot(const KryArgs a, const double *w, double *partials) {
    __shared__ double red[16];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int x0 = 2 * p;
    const bool half = x0 + 1 == a.nx;
    double acc[KB];
#pragma unroll
    for (int i = 0; i < KB; i++) acc[i] = 0.0;
    if (p < a.npairs) {
        KRY_ROWS(a) {
            const long o = kry_row_offset(a, row) + x0;
            double2 vv[KB];
#pragma unroll
            for (int i = 0; i < KB; i++) vv[i] = ld2(a.v[i] + o, i < a.k);
            const double2 wv = ld2(w + o, true);
#pragma unroll
            for (int i = 0; i < KB; i++) {
                const double px = vv[i].x * wv.x, py = half ? 0.0 : vv[i].y * wv.y;
                acc[i] += px + py;
            }
        }
    }
    const int blk = blockIdx.y * gridDim.x + blockIdx.x, nblk = gridDim.x * gridDim.y;
#pragma unroll
    for (int i = 0; i < KB; i++) {
        if (i < a.k) {                                  // uniform over the block
            const double s = block_sum(acc[i], red);
            if (threadIdx.x == 0) partials[(long)i * nblk + blk] = s;
        }
    }
}

template <int KB>
__global__ void __launch_bounds__(256) k_multi_axpy_sumsq(const KryArgs a, const double *h, double *w, double *partials) {
    __shared__ double red[16];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int x0 = 2 * p;
    const bool half = x0 + 1 == a.nx, nt = kry_nt(a);
    double hh[KB];
#pragma unroll
    for (int i = 0; i < KB; i++) hh[i] = i < a.k ? h[i] : 0.0;
    double acc = 0.0;
    if (p < a.npairs) {
        KRY_ROWS(a) {
            const long o = kry_row_offset(a, row) + x0;
            double2 vv[KB];
#pragma unroll
            for (int i = 0; i < KB; i++) vv[i] = ld2(a.v[i] + o, i < a.k);
            double2 wv = ld2(w + o, true);
#pragma unroll
            for (int i = 0; i < KB; i++) {
                if (i < a.k) {
                    const double tx = hh[i] * vv[i].x, ty = hh[i] * vv[i].y;
                    wv.x = wv.x - tx; wv.y = wv.y - ty;
                }
            }
            kry_store(w + o, wv, half, nt);
            const double px = wv.x * wv.x, py = half ? 0.0 : wv.y * wv.y;
            acc += px + py;
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

template <int KB>
__global__ void __launch_bounds__(256) k_lincomb(const KryArgs a, const KryCoefs c, double *out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.npairs) return;
    const int x0 = 2 * p;
    const bool half = x0 + 1 == a.nx, nt = kry_nt(a);
    KRY_ROWS(a) {
        const long o = kry_row_offset(a, row) + x0;
        double2 vv[KB];
#pragma unroll
        for (int i = 0; i < KB; i++) vv[i] = ld2(a.v[i] + o, i < a.k);
        double2 t;
        t.x = c.y[0] * vv[0].x; t.y = c.y[0] * vv[0].y;
#pragma unroll
        for (int i = 1; i < KB; i++) {
            if (i < a.k) {
                const double tx = c.y[i] * vv[i].x, ty = c.y[i] * vv[i].y;
                t.x = t.x + tx; t.y = t.y + ty;
            }
        }
        kry_store(out + o, t, half, nt);
    }
}

__global__ void __launch_bounds__(256) k_scale_to(const KryArgs a, double f, const double *x, double *out, double *out2) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.npairs) return;
    const int x0 = 2 * p;
    const bool half = x0 + 1 == a.nx, nt = kry_nt(a);
    KRY_ROWS(a) {
        const long o = kry_row_offset(a, row) + x0;
        const double2 xv = ld2(x + o, true);
        double2 t;
        t.x = f * xv.x; t.y = f * xv.y;
        kry_store(out + o, t, half, nt);
        if (out2) kry_store(out2 + o, t, half, nt);
    }
}

// value q (one block each) = the partials [q * n, (q + 1) * n) summed in a fixed order
__global__ void __launch_bounds__(256) k_kry_finish(const double *partials, int n, double *out) {
    __shared__ double red[16];
    const double *pp = partials + (long)blockIdx.x * n;
    double s = 0.0;
    for (int q = threadIdx.x; q < n; q += 256) s += pp[q];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

const int KRY_MAX_BLOCKS = 1024;            // x MGK_KRYLOV_MAX partials fit the context's 3 x 16384 slots

int kry_args(KryArgs &a, const mgk_geom *g, int k, const double *const *v) {
    memset(&a, 0, sizeof(a));
    a.nx = g->nx; a.ny = g->ny; a.npairs = (g->nx + 1) / 2; a.k = k;
    a.pitch = g->pitch; a.plane = g->plane; a.nrows = (long)g->ny * g->nz;
    a.nt = store_policy();
    for (int i = 0; i < MGK_KRYLOV_MAX; i++) {
        if (i < k && !v[i]) return 1;
        a.v[i] = i < k ? v[i] + g->org : nullptr;
    }
    return 0;
}
void kry_grid(const KryArgs &a, dim3 &grid, dim3 &block) {
    block = dim3(256);
    const unsigned gx = (a.npairs + 255) / 256;
    long gy = a.nrows, cap = KRY_MAX_BLOCKS / (long)gx;
    if (cap < 1) cap = 1;
    if (gy > cap) gy = cap;
    grid = dim3(gx, (unsigned)gy);
}
bool kry_geom_ok(const mgk_geom *g) {
    return g && (g->dim == 2 || g->dim == 3) && g->nx >= 1 && g->ny >= 1 && g->nz >= 1 && (g->nx & 1) && (g->nx + 1) / 2 <= 256 * KRY_MAX_BLOCKS;
}

// the smallest built width that holds k operands
#define KRY_DISPATCH(k, CALL)                                        \
    do {                                                             \
        if ((k) <= 1) { CALL(1); } else if ((k) <= 2) { CALL(2); }   \
        else if ((k) <= 4) { CALL(4); } else if ((k) <= 8) { CALL(8); } \
        else if ((k) <= 16) { CALL(16); } else if ((k) <= 24) { CALL(24); } \
        else { CALL(MGK_KRYLOV_MAX); }                               \
    } while (0)

}  // namespace

MGK_PRELOAD_UNIT(k_kry_finish)

extern "C" int mgk_multi_dot_f64(mgk_ctx *c, const mgk_geom *g, int k, const double *const *v, const double *w, double *out_dev,
                                 double *out_host, void *stream) {
    if (!c || !kry_geom_ok(g) || k < 1 || k > MGK_KRYLOV_MAX || !v || !w || !out_dev) return fail(MGK_EINVAL, "mgk_multi_dot_f64: bad arguments");
    KryArgs a;
    if (kry_args(a, g, k, v)) return fail(MGK_EINVAL, "mgk_multi_dot_f64: null operand");
    dim3 grid, block;
    kry_grid(a, grid, block);
    const int nblk = (int)(grid.x * grid.y);
    if ((long)k * nblk > 3L * c->max_partials) return fail(MGK_EINVAL, "mgk_multi_dot_f64: more partials than slots");
    hipStream_t s = S(c, stream);
#define CALL(KB) hipLaunchKernelGGL(k_multi_dot<KB>, grid, block, 0, s, a, w + g->org, c->partials)
    KRY_DISPATCH(k, CALL);
#undef CALL
    hipLaunchKernelGGL(k_kry_finish, dim3(k), dim3(256), 0, s, c->partials, nblk, out_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->result_host, out_dev, sizeof(double) * k, hipMemcpyDeviceToHost, s));
    if (out_host) {
        HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < k; i++) out_host[i] = c->result_host[i];
    }
    return 0;
}

extern "C" int mgk_multi_axpy_sumsq_f64(mgk_ctx *c, const mgk_geom *g, int k, const double *h_dev, const double *const *v, double *w,
                                        double *sumsq_host, void *stream) {
    if (!c || !kry_geom_ok(g) || k < 1 || k > MGK_KRYLOV_MAX || !h_dev || !v || !w) return fail(MGK_EINVAL, "mgk_multi_axpy_sumsq_f64: bad arguments");
    KryArgs a;
    if (kry_args(a, g, k, v)) return fail(MGK_EINVAL, "mgk_multi_axpy_sumsq_f64: null operand");
    for (int i = 0; i < k; i++) if (v[i] == w) return fail(MGK_EINVAL, "mgk_multi_axpy_sumsq_f64: w is one of the operands");
    dim3 grid, block;
    kry_grid(a, grid, block);
    if ((long)grid.x * grid.y > c->max_partials) return fail(MGK_EINVAL, "mgk_multi_axpy_sumsq_f64: more blocks than partial slots");
    hipStream_t s = S(c, stream);
#define CALL(KB) hipLaunchKernelGGL(k_multi_axpy_sumsq<KB>, grid, block, 0, s, a, h_dev, w + g->org, c->partials)
    KRY_DISPATCH(k, CALL);
#undef CALL
    double *slot = c->result_dev + MGK_KRYLOV_MAX;
    hipLaunchKernelGGL(k_kry_finish, dim3(1), dim3(256), 0, s, c->partials, (int)(grid.x * grid.y), slot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->result_host + MGK_KRYLOV_MAX, slot, sizeof(double), hipMemcpyDeviceToHost, s));
    if (sumsq_host) {
        HIPCHK(hipStreamSynchronize(s));
        *sumsq_host = c->result_host[MGK_KRYLOV_MAX];
    }
    return 0;
}

extern "C" int mgk_krylov_fetch(mgk_ctx *c, int k, double *h_host, double *sumsq_host, void *stream) {
    if (!c || k < 0 || k > MGK_KRYLOV_MAX || (k > 0 && !h_host)) return fail(MGK_EINVAL, "mgk_krylov_fetch: bad arguments");
    HIPCHK(hipStreamSynchronize(S(c, stream)));
    for (int i = 0; i < k; i++) h_host[i] = c->result_host[i];
    if (sumsq_host) *sumsq_host = c->result_host[MGK_KRYLOV_MAX];
    return 0;
}

extern "C" int mgk_lincomb_f64(mgk_ctx *c, const mgk_geom *g, int k, const double *y, const double *const *v, double *out, void *stream) {
    if (!c || !kry_geom_ok(g) || k < 1 || k > MGK_KRYLOV_MAX || !y || !v || !out) return fail(MGK_EINVAL, "mgk_lincomb_f64: bad arguments");
    KryArgs a;
    if (kry_args(a, g, k, v)) return fail(MGK_EINVAL, "mgk_lincomb_f64: null operand");
    for (int i = 0; i < k; i++) if (v[i] == out) return fail(MGK_EINVAL, "mgk_lincomb_f64: out is one of the operands");
    KryCoefs cf; memset(&cf, 0, sizeof(cf));
    for (int i = 0; i < k; i++) cf.y[i] = y[i];
    dim3 grid, block;
    kry_grid(a, grid, block);
#define CALL(KB) hipLaunchKernelGGL(k_lincomb<KB>, grid, block, 0, S(c, stream), a, cf, out + g->org)
    KRY_DISPATCH(k, CALL);
#undef CALL
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mgk_scale_to_f64(mgk_ctx *c, const mgk_geom *g, double f, const double *x, double *out, double *out2, void *stream) {
    if (!c || !kry_geom_ok(g) || !x || !out || out == out2) return fail(MGK_EINVAL, "mgk_scale_to_f64: bad arguments");
    KryArgs a;
    kry_args(a, g, 0, nullptr);
    dim3 grid, block;
    kry_grid(a, grid, block);
    hipLaunchKernelGGL(k_scale_to, grid, block, 0, S(c, stream), a, f, x + g->org, out + g->org, out2 ? out2 + g->org : nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}
