// mgk_tail.hip -- the tail of the hierarchy in ONE launch: the levels with n <= 15 (3-D) / n <= 63 (2-D) resident in LDS, walked by one
// 1024-lane workgroup: k_tail (V-cycle, Richardson + Jacobi), k_tail_cheby (Chebyshev smoothing), k_tail_fmg (full multigrid), the launcher
// tail_cycle and the entry points mgk_tail_*; mgk_debug_tail_stamps and its per-thread pointer, which mgk_line_tail.hip reads too.
// tail_stencil and tail_cheby_step are NOT __forceinline__: they stay in one module with all their callers.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off   (NO fast-math: each operation evaluates exactly the expressions of the kernels
// it replaces, so the cycle stays bit-identical).
//
// Reference operations replaced (paths relative to the reference's root):
//   k_tail*            the coarse levels' share of the V-cycle loop     src/solver.c:1533-1544
//
// Takes from other units: nothing but the shared headers.  Gives: g_tail_stamps (mgk_tail_dev.hpp).
#include "mgk_dev.hpp"
#include "mgk_tail_dev.hpp"        // MGK_TAIL_MAXLEV, tail_idx, tail_points, tail_restrict, tail_prolong_add
#include <type_traits>
#include "mg_cheby_coefs.h"

// ------------------------------------------------------------------------------------------
// The tail of the hierarchy in ONE kernel: the levels with n <= 15 (3-D) / n <= 63 (2-D) hold at most a few thousand
// unknowns each; their part of a V-cycle is ~50 launches of ~4.5 us of which the arithmetic is a rounding error.  One
// 1024-lane workgroup keeps u, its ping-pong partner and b of EVERY tail level in LDS (ghost rings included: 139 KB in 3-D,
// 137 KB in 2-D) and walks the reference's loop (src/solver.c:1533-1544) over them with a workgroup barrier between
// operations.  Each operation evaluates exactly the expressions of the kernels it replaces (k_stencil / k_jacobi_zero /
// k_restrict / k_prolong_add: same terms, same order, no FMA), so the cycle stays bit-identical.
// In: b of the first tail level (global, padded layout; produced by the restriction from the level above).
// Out: u of that level after its post-smoothing (global), ready for the prolongation to the level above.
// ------------------------------------------------------------------------------------------
#define MGK_TAIL_LDS_BYTES 143360          /* 140 KiB of the 160 KiB */
template <typename T>
struct TailArgs {
    int dim, nlev, v0, v1;
    int n[MGK_TAIL_MAXLEV];
    int off[MGK_TAIL_MAXLEV];              // offset (elements) of the level's three arrays in LDS: A0, A1 (u ping-pong), B; each (n+2)^dim
    T coef[MGK_TAIL_MAXLEV][7], dinv[MGK_TAIL_MAXLEV];
    T scale, cscale;                       // the Richardson damping factor; cscale: on the COARSEST level (PCMG's exact solve of a 1 x 1 system is one undamped sweep)
    const T *b_in;
    T *u_out;                              // both at the interior origin of the first tail level's padded field
    long rs, ms;                           // its row / plane strides
    int total;                             // elements of LDS in use
    const T *ctab[MGK_TAIL_MAXLEV], *dtab[MGK_TAIL_MAXLEV];   // optional (2-D stretched meshes): per-row coefficients / 1/diag of every tail level
    long long *stamps;                     // profiling aid (mgk_debug_tail_stamps; null in production): lane 0 deposits s_memrealtime / s_memtime pairs at every barrier
};

// mode 0: out = u + scale*((b - A u)*dinv); mode 1: out = b - A u; mode 2 (zero guess): out = scale*(b*dinv)
template <typename T, int DIM>
__device__ void tail_stencil(int mode, int n, const T *cf_, T dinv_, T scale, const T *u, const T *b, T *out, const T *ctab = nullptr, const T *dtab = nullptr) {
    const int m = n + 2, sk = m * m;
    tail_points<DIM>(n, [&](int k, int i, int j) {
        const int q = tail_idx<T, DIM>(m, k, i, j);
        const T *cf = (DIM == 2 && ctab) ? ctab + 5 * i : cf_;
        const T dinv = (DIM == 2 && dtab) ? dtab[i] : dinv_;
        if (mode == 2) { const T zx = b[q] * dinv; out[q] = scale * zx; return; }
        T t;
        if (DIM == 3) {
            t = cf[0] * u[q - sk];
            t = t + cf[1] * u[q - m];
            t = t + cf[2] * u[q - 1];
            t = t + cf[3] * u[q];
            t = t + cf[4] * u[q + 1];
            t = t + cf[5] * u[q + m];
            t = t + cf[6] * u[q + sk];
        } else {
            t = cf[0] * u[q - m];
            t = t + cf[1] * u[q - 1];
            t = t + cf[2] * u[q];
            t = t + cf[3] * u[q + 1];
            t = t + cf[4] * u[q + m];
        }
        const T res = b[q] - t;
        if (mode == 1) { out[q] = res; return; }
        const T zz = res * dinv;
        out[q] = u[q] + scale * zz;
    });
}

template <typename T, int DIM>
__global__ void __launch_bounds__(1024) k_tail(const TailArgs<T> a) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[MGK_TAIL_LDS_BYTES];
    T *lds = reinterpret_cast<T *>(raw);
    int nstamp = 0;
    auto stamp = [&]() { if (a.stamps && threadIdx.x == 0 && nstamp < 128) { a.stamps[2 * nstamp] = wall_clock64(); a.stamps[2 * nstamp + 1] = clock64(); nstamp++; } };
    stamp();
    for (int q = threadIdx.x; q < a.total; q += blockDim.x) lds[q] = (T)0;        // ghost rings stay 0 (homogeneous Dirichlet)
    __syncthreads();
    stamp();
    int cur[MGK_TAIL_MAXLEV];                     // which of A0 / A1 holds u of the level
    auto A = [&](int l, int which) -> T * { const int m = a.n[l] + 2; const int sz = (DIM == 3) ? m * m * m : m * m; return lds + a.off[l] + which * sz; };
    auto Bv = [&](int l) -> T * { return A(l, 2); };
    {   // b of the first tail level from global memory
        const int n = a.n[0], m = n + 2, N = (DIM == 3) ? n * n * n : n * n;
        T *b0 = Bv(0);
        for (int p = threadIdx.x; p < N; p += blockDim.x) {
            const int j = p % n, i = (p / n) % n, k = (DIM == 3) ? p / (n * n) : 0;
            b0[tail_idx<T, DIM>(m, k, i, j)] = a.b_in[(long)k * a.ms + (long)i * a.rs + j];
        }
    }
    __syncthreads(); stamp();
    // KSPSolve from a zero guess, `sweeps` Richardson+Jacobi sweeps (src/solver.c:1536): the first is scale*(b*dinv)
    auto smooth0 = [&](int l, int sweeps) {
        cur[l] = 0;
        if (sweeps < 1) return;                   // KSPSolve zero-fills: A0 is still all zeros
        const T sc = (l == a.nlev - 1) ? a.cscale : a.scale;
        tail_stencil<T, DIM>(2, a.n[l], a.coef[l], a.dinv[l], sc, A(l, 0), Bv(l), A(l, 0), a.ctab[l], a.dtab[l]);
        __syncthreads(); stamp();
        for (int it = 1; it < sweeps; it++) {
            tail_stencil<T, DIM>(0, a.n[l], a.coef[l], a.dinv[l], sc, A(l, cur[l]), Bv(l), A(l, cur[l] ^ 1), a.ctab[l], a.dtab[l]);
            __syncthreads(); stamp();
            cur[l] ^= 1;
        }
    };
    smooth0(0, a.nlev == 1 ? a.v1 : a.v0);
    for (int l = 1; l < a.nlev; l++) {            // :1534-1537
        tail_stencil<T, DIM>(1, a.n[l - 1], a.coef[l - 1], a.dinv[l - 1], a.scale, A(l - 1, cur[l - 1]), Bv(l - 1), A(l - 1, cur[l - 1] ^ 1), a.ctab[l - 1], a.dtab[l - 1]);
        __syncthreads(); stamp();
        tail_restrict<T, DIM>(a.n[l - 1], a.n[l], A(l - 1, cur[l - 1] ^ 1), Bv(l));
        __syncthreads(); stamp();
        // the zero-guess sweep writes A0 of level l, which is all zeros only in the first cycle... it is overwritten in full
        smooth0(l, l == a.nlev - 1 ? a.v1 : a.v0);
    }
    for (int l = a.nlev - 2; l >= 0; l--) {       // :1540-1542
        tail_prolong_add<T, DIM>(a.n[l], a.n[l + 1], A(l + 1, cur[l + 1]), A(l, cur[l]));
        __syncthreads(); stamp();
        for (int it = 0; it < a.v0; it++) {
            tail_stencil<T, DIM>(0, a.n[l], a.coef[l], a.dinv[l], a.scale, A(l, cur[l]), Bv(l), A(l, cur[l] ^ 1), a.ctab[l], a.dtab[l]);
            __syncthreads(); stamp();
            cur[l] ^= 1;
        }
    }
    {
        const int n = a.n[0], m = n + 2, N = (DIM == 3) ? n * n * n : n * n;
        const T *u0 = A(0, cur[0]);
        for (int p = threadIdx.x; p < N; p += blockDim.x) {
            const int j = p % n, i = (p / n) % n, k = (DIM == 3) ? p / (n * n) : 0;
            a.u_out[(long)k * a.ms + (long)i * a.rs + j] = u0[tail_idx<T, DIM>(m, k, i, j)];
        }
    }
    stamp();
    if (a.stamps && threadIdx.x == 0) a.stamps[256] = nstamp;
}

// The tail with KSPCHEBYSHEV on every level (mgk_tail_cycle_cheby_f64; fp64): every KSPSolve is the restarted three-term recurrence of
// k_stencil<MODE_CHEBY> / smooth_chebyshev (mg_solver.c).  Its first step is a sweep with scale s = 2 / (emax + emin) (mode 2 from the
// zero guess, mode 0 otherwise; taken even when the step count is 0, as PETSc's cheby.c does); a further step reads p_k from one array of
// the level's ping-pong pair and p_{k-1} -- at the point itself only -- from the other, and writes p_{k+1} over it: two arrays per level
// suffice.  From the zero guess p_0 is the partner array, all zeros until the level's first solve of this launch.
#define MGK_TAIL_CHEB_MAXIT 16
struct TailChebArgs {
    TailArgs<double> t;
    double s;                                   // scale of the first step
    double c[MGK_TAIL_CHEB_MAXIT - 1][3];       // {1 - omega, omega, omega * Gamma * s} of the steps 2, 3, ...
};
// out = (c_km1 * out + c_k * pk) + c_z * ((b - A pk) * dinv): out holds p_{k-1} and receives p_{k+1}
template <int DIM>
__device__ void tail_cheby_step(int n, const double *cf_, double dinv_, double ckm1, double ck, double cz, const double *pk, const double *b, double *out,
                                const double *ctab, const double *dtab) {
    const int m = n + 2, sk = m * m;
    tail_points<DIM>(n, [&](int k, int i, int j) {
        const int q = tail_idx<double, DIM>(m, k, i, j);
        const double *cf = (DIM == 2 && ctab) ? ctab + 5 * i : cf_;
        const double dinv = (DIM == 2 && dtab) ? dtab[i] : dinv_;
        double t;
        if (DIM == 3) {
            t = cf[0] * pk[q - sk];
            t = t + cf[1] * pk[q - m];
            t = t + cf[2] * pk[q - 1];
            t = t + cf[3] * pk[q];
            t = t + cf[4] * pk[q + 1];
            t = t + cf[5] * pk[q + m];
            t = t + cf[6] * pk[q + sk];
        } else {
            t = cf[0] * pk[q - m];
            t = t + cf[1] * pk[q - 1];
            t = t + cf[2] * pk[q];
            t = t + cf[3] * pk[q + 1];
            t = t + cf[4] * pk[q + m];
        }
        const double res = b[q] - t;
        const double zz = res * dinv;
        out[q] = (ckm1 * out[q] + ck * pk[q]) + cz * zz;
    });
}
template <int DIM>
__global__ void __launch_bounds__(1024) k_tail_cheby(const TailChebArgs ca) {
    using T = double;
    const TailArgs<double> &a = ca.t;
    __shared__ __attribute__((aligned(16))) unsigned char raw[MGK_TAIL_LDS_BYTES];
    T *lds = reinterpret_cast<T *>(raw);
    for (int q = threadIdx.x; q < a.total; q += blockDim.x) lds[q] = (T)0;        // ghost rings stay 0 (homogeneous Dirichlet)
    __syncthreads();
    int cur[MGK_TAIL_MAXLEV];                     // which of A0 / A1 holds u of the level
    auto A = [&](int l, int which) -> T * { const int m = a.n[l] + 2; const int sz = (DIM == 3) ? m * m * m : m * m; return lds + a.off[l] + which * sz; };
    auto Bv = [&](int l) -> T * { return A(l, 2); };
    {   // b of the first tail level from global memory
        const int n = a.n[0], m = n + 2, N = (DIM == 3) ? n * n * n : n * n;
        T *b0 = Bv(0);
        for (int p = threadIdx.x; p < N; p += blockDim.x) {
            const int j = p % n, i = (p / n) % n, k = (DIM == 3) ? p / (n * n) : 0;
            b0[tail_idx<T, DIM>(m, k, i, j)] = a.b_in[(long)k * a.ms + (long)i * a.rs + j];
        }
    }
    __syncthreads();
    // KSPSolve with max_it = steps: from the zero guess (the level's two arrays are still all zeros: A1 is p_0) or from the guess in A(l, cur[l])
    auto solve = [&](int l, int steps, bool zero) {
        if (zero) {
            cur[l] = 0;
            tail_stencil<T, DIM>(2, a.n[l], a.coef[l], a.dinv[l], ca.s, A(l, 0), Bv(l), A(l, 0), a.ctab[l], a.dtab[l]);
        } else {
            tail_stencil<T, DIM>(0, a.n[l], a.coef[l], a.dinv[l], ca.s, A(l, cur[l]), Bv(l), A(l, cur[l] ^ 1), a.ctab[l], a.dtab[l]);
            cur[l] ^= 1;
        }
        __syncthreads();
        for (int it = 1; it < steps; it++) {
            tail_cheby_step<DIM>(a.n[l], a.coef[l], a.dinv[l], ca.c[it - 1][0], ca.c[it - 1][1], ca.c[it - 1][2], A(l, cur[l]), Bv(l), A(l, cur[l] ^ 1),
                                 a.ctab[l], a.dtab[l]);
            __syncthreads();
            cur[l] ^= 1;
        }
    };
    solve(0, a.nlev == 1 ? a.v1 : a.v0, true);
    for (int l = 1; l < a.nlev; l++) {            // :1534-1537
        tail_stencil<T, DIM>(1, a.n[l - 1], a.coef[l - 1], a.dinv[l - 1], ca.s, A(l - 1, cur[l - 1]), Bv(l - 1), A(l - 1, cur[l - 1] ^ 1), a.ctab[l - 1], a.dtab[l - 1]);
        __syncthreads();
        tail_restrict<T, DIM>(a.n[l - 1], a.n[l], A(l - 1, cur[l - 1] ^ 1), Bv(l));
        __syncthreads();
        solve(l, l == a.nlev - 1 ? a.v1 : a.v0, true);
    }
    for (int l = a.nlev - 2; l >= 0; l--) {       // :1540-1542
        tail_prolong_add<T, DIM>(a.n[l], a.n[l + 1], A(l + 1, cur[l + 1]), A(l, cur[l]));
        __syncthreads();
        solve(l, a.v0, false);
    }
    {
        const int n = a.n[0], m = n + 2, N = (DIM == 3) ? n * n * n : n * n;
        const T *u0 = A(0, cur[0]);
        for (int p = threadIdx.x; p < N; p += blockDim.x) {
            const int j = p % n, i = (p / n) % n, k = (DIM == 3) ? p / (n * n) : 0;
            a.u_out[(long)k * a.ms + (long)i * a.rs + j] = u0[tail_idx<T, DIM>(m, k, i, j)];
        }
    }
}

// Full multigrid on the tail levels (mgk_tail_fmg_f64), one launch: b of the first tail level comes in, the FMG restriction chain
// b_l = R b_{l-1} runs down, the coarsest level gets v1 sweeps from the zero guess, and for every root r = nlev-2 .. 0: u_r = 0 + P u_{r+1}
// (level r's arrays are untouched until its stage: A0 is still all zeros), then nu V-cycles on the levels r .. nlev-1 -- v0 sweeps on r from
// that guess, residual + restriction + zero-guess sweeps down, prolongation + v0 sweeps up (the operations of k_tail, in the order of the
// host's cycle).  u of the first tail level goes out.
template <typename T, int DIM>
__global__ void __launch_bounds__(1024) k_tail_fmg(const TailArgs<T> a, int nu) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[MGK_TAIL_LDS_BYTES];
    T *lds = reinterpret_cast<T *>(raw);
    for (int q = threadIdx.x; q < a.total; q += blockDim.x) lds[q] = (T)0;        // ghost rings stay 0 (homogeneous Dirichlet)
    __syncthreads();
    int cur[MGK_TAIL_MAXLEV];
    auto A = [&](int l, int which) -> T * { const int m = a.n[l] + 2; const int sz = (DIM == 3) ? m * m * m : m * m; return lds + a.off[l] + which * sz; };
    auto Bv = [&](int l) -> T * { return A(l, 2); };
    {
        const int n = a.n[0], m = n + 2, N = (DIM == 3) ? n * n * n : n * n;
        T *b0 = Bv(0);
        for (int p = threadIdx.x; p < N; p += blockDim.x) {
            const int j = p % n, i = (p / n) % n, k = (DIM == 3) ? p / (n * n) : 0;
            b0[tail_idx<T, DIM>(m, k, i, j)] = a.b_in[(long)k * a.ms + (long)i * a.rs + j];
        }
    }
    __syncthreads();
    for (int l = 1; l < a.nlev; l++) {            // b_l = R b_{l-1}
        tail_restrict<T, DIM>(a.n[l - 1], a.n[l], Bv(l - 1), Bv(l));
        __syncthreads();
    }
    // KSPSolve from a zero guess: the first sweep is scale*(b*dinv); with no sweep at all the level is zero-filled (A0 may hold an earlier stage's u)
    auto smooth0 = [&](int l, int sweeps) {
        cur[l] = 0;
        const T sc = (l == a.nlev - 1) ? a.cscale : a.scale;
        if (sweeps < 1) {
            tail_points<DIM>(a.n[l], [&](int k, int i, int j) { A(l, 0)[tail_idx<T, DIM>(a.n[l] + 2, k, i, j)] = (T)0; });
            __syncthreads();
            return;
        }
        tail_stencil<T, DIM>(2, a.n[l], a.coef[l], a.dinv[l], sc, A(l, 0), Bv(l), A(l, 0));
        __syncthreads();
        for (int it = 1; it < sweeps; it++) {
            tail_stencil<T, DIM>(0, a.n[l], a.coef[l], a.dinv[l], sc, A(l, cur[l]), Bv(l), A(l, cur[l] ^ 1));
            __syncthreads();
            cur[l] ^= 1;
        }
    };
    auto sweeps = [&](int l, int count) {         // from the guess in A(l, cur[l])
        for (int it = 0; it < count; it++) {
            tail_stencil<T, DIM>(0, a.n[l], a.coef[l], a.dinv[l], a.scale, A(l, cur[l]), Bv(l), A(l, cur[l] ^ 1));
            __syncthreads();
            cur[l] ^= 1;
        }
    };
    smooth0(a.nlev - 1, a.v1);
    for (int r = a.nlev - 2; r >= 0; r--) {
        cur[r] = 0;
        tail_prolong_add<T, DIM>(a.n[r], a.n[r + 1], A(r + 1, cur[r + 1]), A(r, 0));    // 0 + P u_{r+1}
        __syncthreads();
        for (int c = 0; c < nu; c++) {
            sweeps(r, a.v0);
            for (int l = r + 1; l < a.nlev; l++) {
                tail_stencil<T, DIM>(1, a.n[l - 1], a.coef[l - 1], a.dinv[l - 1], a.scale, A(l - 1, cur[l - 1]), Bv(l - 1), A(l - 1, cur[l - 1] ^ 1));
                __syncthreads();
                tail_restrict<T, DIM>(a.n[l - 1], a.n[l], A(l - 1, cur[l - 1] ^ 1), Bv(l));
                __syncthreads();
                smooth0(l, l == a.nlev - 1 ? a.v1 : a.v0);
            }
            for (int l = a.nlev - 2; l >= r; l--) {
                tail_prolong_add<T, DIM>(a.n[l], a.n[l + 1], A(l + 1, cur[l + 1]), A(l, cur[l]));
                __syncthreads();
                sweeps(l, a.v0);
            }
        }
    }
    {
        const int n = a.n[0], m = n + 2, N = (DIM == 3) ? n * n * n : n * n;
        const T *u0 = A(0, cur[0]);
        for (int p = threadIdx.x; p < N; p += blockDim.x) {
            const int j = p % n, i = (p / n) % n, k = (DIM == 3) ? p / (n * n) : 0;
            a.u_out[(long)k * a.ms + (long)i * a.rs + j] = u0[tail_idx<T, DIM>(m, k, i, j)];
        }
    }
}

thread_local long long *g_tail_stamps = nullptr;      // (read by mgk_line_tail.hip too: mgk_tail_dev.hpp)
// profiling aid: the tail kernels launched by this thread deposit (s_memrealtime, s_memtime) at each of their barriers into dev[0 .. 255]
// and the number of pairs into dev[256] (257 long longs of device memory; null switches it off)
extern "C" void mgk_debug_tail_stamps(long long *dev) { g_tail_stamps = dev; }
template <typename T>
static int tail_cycle(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, const double *coef7, const double *dinv, double scale,
                      int v0, int v1, const T *b, T *u, void *stream, const T *const *ctab = nullptr, const T *const *dtab = nullptr, const double *cscale = nullptr,
                      int fmg_nu = 0, const double *cheb_eig = nullptr) {
    if (!c || !g0 || !n || (!coef7 && !ctab) || (!dinv && !dtab) || !b || !u || nlev < 1 || nlev > MGK_TAIL_MAXLEV || v0 < 0 || v1 < 0 ||
        (ctab && (!dtab || g0->dim != 2)))
        return fail(MGK_EINVAL, "mgk_tail_cycle: bad arguments");
    if (n[0] != g0->nx || g0->ny != g0->nx || (g0->dim == 3 && g0->nz != g0->nx))
        return fail(MGK_EINVAL, "mgk_tail_cycle: the first tail level must be a whole cube / square of n[0] unknowns per side");
    TailArgs<T> a; memset(&a, 0, sizeof(a));
    a.dim = g0->dim; a.nlev = nlev; a.v0 = v0; a.v1 = v1; a.scale = (T)scale; a.cscale = (T)(cscale ? *cscale : scale);
    long off = 0;
    for (int l = 0; l < nlev; l++) {
        if (n[l] < 1 || (l > 0 && n[l - 1] != 2 * n[l] + 1)) return fail(MGK_EINVAL, "mgk_tail_cycle: need n[l-1] = 2 n[l] + 1");
        const long m = n[l] + 2, sz = (g0->dim == 3) ? m * m * m : m * m;
        a.n[l] = n[l]; a.off[l] = (int)off; off += 3 * sz;
        for (int q = 0; q < 7; q++) a.coef[l][q] = coef7 ? (T)coef7[7 * l + q] : (T)0;
        a.dinv[l] = dinv ? (T)dinv[l] : (T)1;
        a.ctab[l] = ctab ? ctab[l] : nullptr; a.dtab[l] = dtab ? dtab[l] : nullptr;
        if (ctab && (!ctab[l] || !dtab[l])) return fail(MGK_EINVAL, "mgk_tail_cycle: null coefficient table");
    }
    if (off * (long)sizeof(T) > MGK_TAIL_LDS_BYTES) return fail(MGK_EINVAL, "mgk_tail_cycle: the levels do not fit in LDS");
    a.total = (int)off;
    a.b_in = b + g0->org; a.u_out = u + g0->org; a.rs = g0->pitch; a.ms = g0->plane;
    a.stamps = g_tail_stamps;
    if constexpr (std::is_same<T, double>::value) {
        if (cheb_eig) {
            // Chebyshev: the step factors of the longest solve, evaluated here with the expressions of smooth_chebyshev (mg_cheby_begin / _next)
            const int steps = v0 > v1 ? v0 : v1;
            if (steps > MGK_TAIL_CHEB_MAXIT || !(cheb_eig[1] > cheb_eig[0] && cheb_eig[0] > 0.0))
                return fail(MGK_EINVAL, "mgk_tail_cycle_cheby_f64: need 0 < emin < emax and at most 16 steps per solve");
            TailChebArgs ca; memset(&ca, 0, sizeof(ca));
            ca.t = a; ca.t.stamps = nullptr;
            mg_cheby_rec rec;
            mg_cheby_begin(&rec, cheb_eig[0], cheb_eig[1]);
            ca.s = rec.scale;
            for (int it = 1; it < steps; it++) mg_cheby_next(&rec, ca.c[it - 1]);
            if (g0->dim == 3) hipLaunchKernelGGL((k_tail_cheby<3>), dim3(1), dim3(1024), 0, S(c, stream), ca);
            else hipLaunchKernelGGL((k_tail_cheby<2>), dim3(1), dim3(1024), 0, S(c, stream), ca);
            HIPCHK(hipGetLastError());
            return 0;
        }
    }
    if (fmg_nu > 0) {
        if (g0->dim == 3) hipLaunchKernelGGL((k_tail_fmg<T, 3>), dim3(1), dim3(1024), 0, S(c, stream), a, fmg_nu);
        else hipLaunchKernelGGL((k_tail_fmg<T, 2>), dim3(1), dim3(1024), 0, S(c, stream), a, fmg_nu);
    } else if (g0->dim == 3) hipLaunchKernelGGL((k_tail<T, 3>), dim3(1), dim3(1024), 0, S(c, stream), a);
    else hipLaunchKernelGGL((k_tail<T, 2>), dim3(1), dim3(1024), 0, S(c, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int mgk_tail_cycle_f64(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, const double *coef7, const double *dinv,
                                  double scale, int v0, int v1, const double *b, double *u, void *stream) {
    return tail_cycle<double>(c, g0, nlev, n, coef7, dinv, scale, v0, v1, b, u, stream);
}
extern "C" int mgk_tail_cycle_f32(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, const double *coef7, const double *dinv,
                                  double scale, int v0, int v1, const float *b, float *u, void *stream) {
    return tail_cycle<float>(c, g0, nlev, n, coef7, dinv, scale, v0, v1, b, u, stream);
}
// 2-D stretched meshes: ctab[l] / dtab[l] are the device tables (n[l] x 5 and n[l] doubles) of tail level l
extern "C" int mgk_tail_cycle_rowcoef_f64(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, const double *const *ctab, const double *const *dtab,
                                          double scale, int v0, int v1, const double *b, double *u, void *stream) {
    if (!ctab || !dtab) return fail(MGK_EINVAL, "mgk_tail_cycle_rowcoef_f64: null tables");
    return tail_cycle<double>(c, g0, nlev, n, nullptr, nullptr, scale, v0, v1, b, u, stream, ctab, dtab);
}
// ... with another damping factor on the COARSEST level (2-D, fp64; constant coefficients or row tables: pass either coef7 + dinv or ctab + dtab):
// PCMG's default coarse solver is exact, and on a 1 x 1 grid the exact solve IS one undamped Jacobi sweep from the zero guess (v1 = 1, coarse_scale = 1)
extern "C" int mgk_tail_cycle_cs_f64(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, const double *coef7, const double *dinv,
                                     const double *const *ctab, const double *const *dtab, double scale, double coarse_scale, int v0, int v1,
                                     const double *b, double *u, void *stream) {
    if ((ctab == nullptr) != (dtab == nullptr)) return fail(MGK_EINVAL, "mgk_tail_cycle_cs_f64: ctab and dtab go together");
    return tail_cycle<double>(c, g0, nlev, n, ctab ? nullptr : coef7, ctab ? nullptr : dinv, scale, v0, v1, b, u, stream, ctab, dtab, &coarse_scale);
}
// ... with KSPCHEBYSHEV (eigenvalue bounds emin, emax) as every level's solver: k_tail_cheby.  2-D and 3-D; either coef7 + dinv or the
// row tables (2-D); any v0, v1 in 0 .. 16
extern "C" int mgk_tail_cycle_cheby_f64(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, const double *coef7, const double *dinv,
                                        const double *const *ctab, const double *const *dtab, double emin, double emax, int v0, int v1,
                                        const double *b, double *u, void *stream) {
    if ((ctab == nullptr) != (dtab == nullptr)) return fail(MGK_EINVAL, "mgk_tail_cycle_cheby_f64: ctab and dtab go together");
    const double eig[2] = {emin, emax};
    return tail_cycle<double>(c, g0, nlev, n, ctab ? nullptr : coef7, ctab ? nullptr : dinv, 1.0, v0, v1, b, u, stream, ctab, dtab, nullptr, 0, eig);
}
extern "C" int mgk_tail_max_n(int dim) { return dim == 3 ? 15 : 63; }
// FMG(nu) on the tail levels in one launch (k_tail_fmg): b of the first tail level in, its u after the stage rooted there out
extern "C" int mgk_tail_fmg_f64(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, const double *coef7, const double *dinv,
                                double scale, int v0, int v1, int nu, const double *b, double *u, void *stream) {
    if (nu < 1 || nlev < 2 || b == u) return fail(MGK_EINVAL, "mgk_tail_fmg_f64: need nu >= 1, two levels or more, b != u");
    return tail_cycle<double>(c, g0, nlev, n, coef7, dinv, scale, v0, v1, b, u, stream, nullptr, nullptr, nullptr, nu);
}

MGK_PRELOAD_UNIT(k_tail<double, 2>)
