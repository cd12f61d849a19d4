// mgk_line_tail.hip -- the LDS-resident coarse levels of a LINE cycle in one launch: mgk_tail_cycle_line_f64, the
// contract of mgk_tail_cycle_f64 (mgk_tail.hip, k_tail) with line sweeps as the smoother.  One workgroup of 1024 lanes keeps u, z and b of
// every tail level in LDS, ghost rings included, and walks the loop of src/solver.c:1533-1544 over them with a workgroup barrier between
// dependent phases.  fp64, no FMA (-ffp-contract=off), no inline assembly; bit-identical to the launch-by-launch loop over mgk_line_* /
// mgk_xline_* / the residual, restriction and prolongation kernels (the definitions: tests/line_reference.py, tests/xline_reference.py).
//
// LDS.  A line sweep swaps nothing, so a level needs three (n+2)^2 arrays: U, Z and B -- k_tail's A0 / A1 / B.  Z holds z of a sweep and
// the residual that feeds the restriction.  With n[0] = 63 and six levels that is 3 x 5718 doubles = 137 232 B.  Beside them sit the tables
// of every level: the row coefficients (5 n), l, g, q of the y sweep (n each) and, on the uniform mesh, the ONE row of the x table (n):
// 9 x 120 doubles = 8 640 B.  Together 145 872 B -- above k_tail's 140 KiB, so this kernel has its own constant (144 KiB of the CU's 160).
// The x table of a stretched level is n rows at a stride of xgs doubles (32 KB at 63^2): it does not fit and is read from global memory.  It
// is read-only for the life of the kernel; a lane walks its own row and asks for a block of it one block ahead of the recurrence.
//
// A sweep is two phases.  (1) ALL lanes: r = b - A u into Z (five terms in the order of tail_stencil mode 1, row table); barrier.  From the
// zero guess r = b: the march reads B instead and the phase is skipped.  (2) ONE lane per line makes the forward march (z into Z) and then the
// backward march of its own line and writes U in place; barrier.  No barrier between the two marches: the lane reads only the z it wrote
// itself, and no lane reads a neighbour's u after the first barrier, which is why the in-place write is safe.
// y sweep: lane = column, a step touches consecutive doubles.  x sweep: lane = row, a stride of n + 2 doubles; n + 2 is odd on every level
// (n = 2^k - 1), so the 32 lanes of a half wave hit 32 different bank pairs: both are conflict-free under the 8-byte bank rule of DESIGN.md
// section 8g.  The dependent chain is one multiply and one subtract per step; everything else a step needs is read ahead of it into
// registers: the LDS operands in blocks of 4 steps, the table values in blocks of 8 (16 from global memory: one 128-byte line), each one
// block ahead, two statically named blocks in turn (no register copies; lt_march).  127 VGPRs, no scratch.
// Ghost rings are zeroed once at the start and never written.  What the phases need of a level -- sizes, offsets, the x table's address --
// sits in LDS too (LtMeta): a run-time index into the argument struct's arrays would send the whole struct to scratch.
#include "mgk_tail_dev.hpp"
#include "mgk_line_dev.hpp"

namespace {

#define MGK_LINE_TAIL_LDS_BYTES 147456     /* 144 KiB of the 160 KiB */
constexpr int LT_Y = 1, LT_X = 2, LT_ALT = 3;      // mg_pc_type's MG_PC_LINE_Y / _X / _ALT (mgk.h does not include mgsolve.h)
constexpr int LB = 4;                              // steps per block of LDS operands

struct LineTailArgs {
    int nlev, v0, v1, pc;
    int n[MGK_TAIL_MAXLEV];
    int off[MGK_TAIL_MAXLEV];              // offset (doubles) of the level's three arrays in LDS: U, Z, B; each (n+2)^2
    int toff[MGK_TAIL_MAXLEV];             // ... of its tables: ct (5 n), l, g, q, x row (n each)
    const double *ctab[MGK_TAIL_MAXLEV], *ltab[MGK_TAIL_MAXLEV], *gtab[MGK_TAIL_MAXLEV], *qtab[MGK_TAIL_MAXLEV], *xgtab[MGK_TAIL_MAXLEV];
    long xgs[MGK_TAIL_MAXLEV];
    double scale;
    const double *b_in;
    double *u_out;                         // both at the interior origin of the first tail level's padded field
    long rs;
    int nfield;                            // doubles of LDS that hold fields (zeroed at the start)
    long long *stamps;                     // profiling aid (mgk_debug_tail_stamps; null in production)
};

struct LtOps { double r[LB], x[LB]; };            // r: r (forward) / z (backward); x: l of a y forward block / u of a backward block from a guess

// the operands of line `t`: MODE 0 a column (y sweep: tables l, g, q in LDS), MODE 1 a row with the x table's one row in LDS (uniform mesh),
// MODE 2 a row with its own row of the x table in global memory.  Step s of the line sits at base + s * st
template <int MODE> __device__ __forceinline__ int lt_base(int m, int t) { return MODE == 0 ? m + t + 1 : (t + 1) * m + 1; }

// The march over `count` steps p = 0 .. count - 1 (count >= 1) of one line, everything off the dependent chain read ahead of it into
// statically indexed registers: the table values (loadG) in blocks of GB steps, one block ahead -- GB = 16 is one 128-byte line of the x table
// in global memory --, the LDS operands (loadL) in blocks of LB steps, one block ahead; two named blocks of each in turn, so nothing is copied.
// A load past the end reads the last step again and a chain step past the end stores nothing (the functors clamp and test).
template <int GB, class FG, class FL, class FC>
__device__ __forceinline__ void lt_march(int count, FG &&loadG, FL &&loadL, FC &&chain) {
    double Ga[GB], Gb[GB];
    LtOps A, B;
    loadG(0, Ga);
    loadL(0, A);
    auto pair = [&](int p0, const double (&g)[GB], auto go) __attribute__((always_inline)) {
        constexpr int GO = decltype(go)::value;
        loadL(p0 + LB, B);
        chain(p0, A, g, line_ic<GO>{});
        loadL(p0 + 2 * LB, A);
        chain(p0 + LB, B, g, line_ic<GO + LB>{});
    };
    auto run = [&](int p0, const double (&g)[GB]) __attribute__((always_inline)) {
        pair(p0, g, line_ic<0>{});
        if constexpr (GB == 16) pair(p0 + 8, g, line_ic<8>{});
    };
    for (int p0 = 0; p0 < count; p0 += 2 * GB) {
        loadG(p0 + GB, Gb);
        run(p0, Ga);
        loadG(p0 + 2 * GB, Ga);
        run(p0 + GB, Gb);
    }
}

// y_0 = r_0, y_s = r_s - l_s y_{s-1}, z_s = y_s g_s; x sweep: l_s = W g_{s-1}, one rounded product (step 0 has no l at all)
template <int MODE>
__device__ __forceinline__ void lt_forward(int n, int t, const double *R, double *Z, const double *ct, const double *lt, const double *G) {
    constexpr int GB = MODE == 2 ? 16 : 8;
    const int m = n + 2, base = lt_base<MODE>(m, t), st = MODE == 0 ? m : 1;
    const double cW = MODE == 0 ? 0.0 : ct[5 * t + 1];
    double gp = G[0], y = R[base];
    Z[base] = y * gp;
    if (n == 1) return;
    const int count = n - 1;                                   // step p is s = 1 + p
    lt_march<GB>(count,
        [&](int p0, double (&g)[GB]) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < GB; k++) g[k] = G[1 + min(p0 + k, count - 1)];
        },
        [&](int p0, LtOps &q) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < LB; k++) {
                const int s = 1 + min(p0 + k, count - 1);
                q.r[k] = R[base + s * st];
                if (MODE == 0) q.x[k] = lt[s];
            }
        },
        [&](int p0, const LtOps &q, const double (&g)[GB], auto go) __attribute__((always_inline)) {
            constexpr int GO = decltype(go)::value;
#pragma unroll
            for (int k = 0; k < LB; k++) {
                const double l = MODE == 0 ? q.x[k] : cW * gp;
                const double ly = l * y;
                y = q.r[k] - ly;
                gp = g[GO + k];
                if (p0 + k < count) Z[base + (1 + p0 + k) * st] = y * gp;
            }
        });
}

// e_{n-1} = z_{n-1}, e_s = z_s - q_s e_{s+1}, u'_s = u_s + scale e_s (ZERO: scale e_s, u is not read); x sweep: q_s = E g_s, one rounded
// product (the last step has no q e at all)
template <int MODE, bool ZERO>
__device__ __forceinline__ void lt_backward(int n, int t, const double *Z, double *U, const double *ct, const double *Q, double scale) {
    constexpr int GB = MODE == 2 ? 16 : 8;
    const int m = n + 2, base = lt_base<MODE>(m, t), st = MODE == 0 ? m : 1;
    const double cE = MODE == 0 ? 0.0 : ct[5 * t + 3];
    const int last = base + (n - 1) * st;
    double e = Z[last];
    {
        const double se = scale * e;
        U[last] = ZERO ? se : U[last] + se;
    }
    if (n == 1) return;
    const int count = n - 1;                                   // step p is s = n - 2 - p
    lt_march<GB>(count,
        [&](int p0, double (&g)[GB]) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < GB; k++) g[k] = Q[n - 2 - min(p0 + k, count - 1)];
        },
        [&](int p0, LtOps &q) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < LB; k++) {
                const int s = n - 2 - min(p0 + k, count - 1);
                q.r[k] = Z[base + s * st];
                if (!ZERO) q.x[k] = U[base + s * st];
            }
        },
        [&](int p0, const LtOps &q, const double (&g)[GB], auto go) __attribute__((always_inline)) {
            constexpr int GO = decltype(go)::value;
#pragma unroll
            for (int k = 0; k < LB; k++) {
                const double qq = MODE == 0 ? g[GO + k] : cE * g[GO + k];
                const double qe = qq * e;
                e = q.r[k] - qe;
                const double se = scale * e;
                if (p0 + k < count) U[base + (n - 2 - p0 - k) * st] = ZERO ? se : q.x[k] + se;
            }
        });
}

template <int MODE>
__device__ __forceinline__ void lt_line(bool zero, int n, int t, const double *R, double *Z, double *U, const double *ct, const double *lt,
                                        const double *G, const double *Q, double scale) {
    lt_forward<MODE>(n, t, R, Z, ct, lt, G);
    if (zero) lt_backward<MODE, true>(n, t, Z, U, ct, Q, scale);
    else lt_backward<MODE, false>(n, t, Z, U, ct, Q, scale);
}

// out = b - A u: the five terms in the order of tail_stencil mode 1, coefficients of the point's grid row
__device__ __forceinline__ void lt_residual(int n, const double *ct, const double *u, const double *b, double *out) {
    const int m = n + 2;
    tail_points<2>(n, [&](int, int i, int j) {
        const int q = tail_idx<double, 2>(m, 0, i, j);
        const double *cf = ct + 5 * i;
        double t = cf[0] * u[q - m];
        t = t + cf[1] * u[q - 1];
        t = t + cf[2] * u[q];
        t = t + cf[3] * u[q + 1];
        t = t + cf[4] * u[q + m];
        out[q] = b[q] - t;
    });
}

// what the phases read of a level, indexed by a level number known only at run time: kept in LDS (a run-time index into the kernel's
// argument arrays would move the whole argument struct to scratch)
struct LtMeta { int n, off, toff; long xgs; const double *xg; };

__global__ void __launch_bounds__(1024) k_tail_line(const LineTailArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[MGK_LINE_TAIL_LDS_BYTES];
    __shared__ LtMeta meta[MGK_TAIL_MAXLEV];
    double *lds = reinterpret_cast<double *>(raw);
    const int t = threadIdx.x;
    int nstamp = 0;
    auto stamp = [&]() { if (a.stamps && t == 0 && nstamp < 128) { a.stamps[2 * nstamp] = wall_clock64(); a.stamps[2 * nstamp + 1] = clock64(); nstamp++; } };
    stamp();
    for (int q = t; q < a.nfield; q += blockDim.x) lds[q] = 0.0;                  // ghost rings stay 0 (homogeneous Dirichlet)
#pragma unroll
    for (int l = 0; l < MGK_TAIL_MAXLEV; l++) {   // static level numbers: the tables of every level into LDS (fields and tables do not overlap)
        if (l >= a.nlev) continue;
        const int n = a.n[l];
        double *tb = lds + a.toff[l];
        if (t == 0) { meta[l].n = n; meta[l].off = a.off[l]; meta[l].toff = a.toff[l]; meta[l].xgs = a.xgs[l]; meta[l].xg = a.xgtab[l]; }
        for (int q = t; q < 5 * n; q += blockDim.x) tb[q] = a.ctab[l][q];
        for (int q = t; q < n; q += blockDim.x) {
            if (a.pc != LT_X) { tb[5 * n + q] = a.ltab[l][q]; tb[6 * n + q] = a.gtab[l][q]; tb[7 * n + q] = a.qtab[l][q]; }
            if (a.pc != LT_Y && a.xgs[l] == 0) tb[8 * n + q] = a.xgtab[l][q];
        }
    }
    __syncthreads();
    stamp();
    auto N = [&](int l) -> int { return meta[l].n; };
    auto U = [&](int l) -> double * { return lds + meta[l].off; };
    auto Z = [&](int l) -> double * { const int m = meta[l].n + 2; return lds + meta[l].off + m * m; };
    auto B = [&](int l) -> double * { const int m = meta[l].n + 2; return lds + meta[l].off + 2 * m * m; };
    auto CT = [&](int l) -> double * { return lds + meta[l].toff; };
    auto TL = [&](int l, int which) -> double * { return lds + meta[l].toff + (5 + which) * meta[l].n; };     // 0 l, 1 g, 2 q, 3 the x row
    {   // b of the first tail level from global memory
        const int n = N(0), m = n + 2;
        double *b0 = B(0);
        tail_points<2>(n, [&](int, int i, int j) { b0[tail_idx<double, 2>(m, 0, i, j)] = a.b_in[(long)i * a.rs + j]; });
    }
    __syncthreads(); stamp();
    // one line sweep of level l, along x or along y, from the zero guess (u is not read: r = b, u' = s e) or from the guess in U
    auto sweep = [&](int l, bool isx, bool zero) __attribute__((always_inline)) {
        const int n = N(l);
        if (!zero) {
            lt_residual(n, CT(l), U(l), B(l), Z(l));
            __syncthreads(); stamp();
        }
        if (t < n) {
            const double *R = zero ? B(l) : Z(l);
            if (!isx) lt_line<0>(zero, n, t, R, Z(l), U(l), CT(l), TL(l, 0), TL(l, 1), TL(l, 2), a.scale);
            else if (meta[l].xgs == 0) lt_line<1>(zero, n, t, R, Z(l), U(l), CT(l), nullptr, TL(l, 3), TL(l, 3), a.scale);
            else {
                const double *gx = meta[l].xg + (long)t * meta[l].xgs;
                lt_line<2>(zero, n, t, R, Z(l), U(l), CT(l), nullptr, gx, gx, a.scale);
            }
        }
        __syncthreads(); stamp();
    };
    // The V-cycle as ONE loop over its stages -- levels 0 .. nlev-1 down, nlev-2 .. 0 up -- so that the sweep is instantiated once.
    // A stage is a KSPSolve with max_it = sweeps: sweep k, counted from 0 in every stage, is an x sweep under LT_X and for odd k under LT_ALT.
    // With no sweep from the zero guess KSPSolve zero-fills: U is still all zeros (a level is smoothed from the zero guess once per launch,
    // before anything wrote it)
    for (int stg = 0; stg < 2 * a.nlev - 1; stg++) {
        const bool down = stg < a.nlev;
        const int l = down ? stg : 2 * a.nlev - 2 - stg;
        if (down && l > 0) {                      // :1534-1535
            lt_residual(N(l - 1), CT(l - 1), U(l - 1), B(l - 1), Z(l - 1));
            __syncthreads(); stamp();
            tail_restrict<double, 2>(N(l - 1), N(l), Z(l - 1), B(l));
            __syncthreads(); stamp();
        }
        if (!down) {                              // :1540-1541
            tail_prolong_add<double, 2>(N(l), N(l + 1), U(l + 1), U(l));
            __syncthreads(); stamp();
        }
        const int sweeps = (down && l == a.nlev - 1) ? a.v1 : a.v0;       // :1531,1536,1542
        for (int k = 0; k < sweeps; k++) sweep(l, a.pc == LT_X || (a.pc == LT_ALT && (k & 1)), down && k == 0);
    }
    {
        const int n = N(0), m = n + 2;
        const double *u0 = U(0);
        tail_points<2>(n, [&](int, int i, int j) { a.u_out[(long)i * a.rs + j] = u0[tail_idx<double, 2>(m, 0, i, j)]; });
    }
    stamp();
    if (a.stamps && t == 0) a.stamps[256] = nstamp;
}

}  // namespace

MGK_PRELOAD_UNIT(k_tail_line)

extern "C" int mgk_tail_cycle_line_f64(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, int pc, const double *const *ctab,
                                       const double *const *ltab, const double *const *gtab, const double *const *qtab,
                                       const double *const *xgtab, const long *xgs, double scale, int v0, int v1, const double *b, double *u,
                                       void *stream) {
    if (!c || !g0 || !n || !ctab || !b || !u || nlev < 1 || nlev > MGK_TAIL_MAXLEV || v0 < 0 || v1 < 0)
        return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: bad arguments (1 to 8 levels, v0 >= 0, v1 >= 0)");
    if (pc != LT_Y && pc != LT_X && pc != LT_ALT)
        return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: pc must be y-line (1), x-line (2) or alternating (3)");
    if (g0->dim != 2 || g0->nz != 1) return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: the line smoothers are 2-D");
    if (n[0] != g0->nx || g0->ny != g0->nx)
        return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: the first tail level must be a whole square of n[0] unknowns per side");
    if (pc != LT_X && (!ltab || !gtab || !qtab)) return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: the y sweeps need ltab, gtab and qtab");
    if (pc != LT_Y && (!xgtab || !xgs)) return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: the x sweeps need xgtab and its row strides");
    LineTailArgs a; memset(&a, 0, sizeof(a));
    a.nlev = nlev; a.v0 = v0; a.v1 = v1; a.pc = pc; a.scale = scale;
    long off = 0, ntab = 0;
    for (int l = 0; l < nlev; l++) {
        if (n[l] < 1 || (l > 0 && n[l - 1] != 2 * n[l] + 1)) return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: need n[l-1] = 2 n[l] + 1");
        if (!ctab[l] || (pc != LT_X && (!ltab[l] || !gtab[l] || !qtab[l])) || (pc != LT_Y && !xgtab[l]))
            return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: null table of a level");
        if (pc != LT_Y && xgs[l] != 0 && xgs[l] < n[l]) return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: an x table's row stride is 0 or at least n");
        const long m = n[l] + 2;
        a.n[l] = n[l]; a.off[l] = (int)off; off += 3 * m * m; ntab += 9 * (long)n[l];
        a.ctab[l] = ctab[l];
        if (pc != LT_X) { a.ltab[l] = ltab[l]; a.gtab[l] = gtab[l]; a.qtab[l] = qtab[l]; }
        if (pc != LT_Y) { a.xgtab[l] = xgtab[l]; a.xgs[l] = xgs[l]; }
    }
    if (n[0] > mgk_tail_max_n(2) || (off + ntab) * (long)sizeof(double) > MGK_LINE_TAIL_LDS_BYTES)
        return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: the levels do not fit in LDS");
    a.nfield = (int)off;
    for (int l = 0; l < nlev; l++) { a.toff[l] = (int)off; off += 9 * (long)n[l]; }
    a.b_in = b + g0->org; a.u_out = u + g0->org; a.rs = g0->pitch;
    a.stamps = g_tail_stamps;
    hipLaunchKernelGGL(k_tail_line, dim3(1), dim3(1024), 0, S(c, stream), a);
    HIPCHK(hipGetLastError());
    return 0;
}
