// mgk_rbgs.hip -- red-black Gauss-Seidel passes, 2-D (pc_type MG_PC_RBGS, csrc/mg_rbgs.c).  Same build flags as every
// unit of libmgk.so (-O3 -ffp-contract=off, gfx950 only); shares mgk_dev.hpp with them.
#include "mgk_dev.hpp"
#include <type_traits>

// ------------------------------------------------------------------------------------------
// One or two red-black Gauss-Seidel sweeps in one pass:
//     plain      unew = RB^nsweeps(u)                     24 B per unknown
//     ZG         from the zero guess: u counts as zero everywhere and is not read     16 B
//     PRO        unew = RB^nsweeps(u + P uc): prolongation, correction and sweeps     25 B
// Point (i, j) (row i, column j, 0-based interior) has the colour (i + j) & 1.  A sweep is two STAGES: stage of colour 0, then of colour 1; a
// stage of colour c replaces every point of colour c by u + scale * ((b - t) * dinv), t the five-term sum of mgk_rowcoef_f64 (S, W, C, E, N;
// no FMA) over the field the stage started from, and passes the other points through.  The four neighbours of a point have the other colour,
// so "from the field the stage started from" IS Gauss-Seidel -- and a pass of NS = 2 nsweeps stages has the dependency shape of a multi-stage
// Jacobi pass: the structure of k_jacobi3_2d (mgk_sweep3.hip).  Every WAVE is independent (no LDS, no barrier).  Lane l holds the column pair
// x0 = 2 ((64 - NS) tx + l - NS / 2); x neighbours come by whole-wavefront DPP shifts.  A stage consumes one column of halo a side, a lane is two
// columns: NS / 2 halo lanes a side, 124 (nsweeps = 1) or 120 (nsweeps = 2) of a wave's 128 columns are stored.  The wave marches along y with
// the last two rows of u and of every stage but the last in registers: at step t stage s (1 .. NS) makes row t + NS - s, the last one stores
// it.  A chunk [y0, y1) starts 2 NS - 2 steps early -- its first row of u is y0 - NS -- with the stages joining in as their rows come to
// matter (wave-uniform branches).
// Colours without a mask: x0 is even, so the element e of a pair on row y has the colour (y + e) & 1, the SAME element in every lane -- and
// stage s on its row t + NS - s updates the element (t + 1) & 1, the same one for all stages of a step.  Chunks start on even rows, the march is
// unrolled by NS: that element is a compile-time constant of the phase, a stage is one stencil sum per lane (not two under a mask) and one
// DPP shift.  The rows live in rings whose ROLES rotate with the phase (no register copies), as in k_jacobi3_2d.
// Every stage forces the positions outside the grid to zero (the homogeneous Dirichlet ring): the result equals the half-sweeps made one
// by one, bit for bit.  Stretched meshes: per-row coefficient tables (TAB) read through the constant address space at wave-uniform
// addresses (scalar loads); a template parameter, not a run-time select (which spilled in k_jacobi3_2d: DESIGN.md section 4 (xv)).
// PRO: the parents of a fine column pair are the coarse columns pidx - 1 and pidx; every lane loads both (lane 0 has no lane to shift the first
// one from, and with one halo lane a side its column c0 matters: on odd rows c0 + 1 is updated from it by the first stage, c0 + 2 -- stored
// -- from that by the second).
// ------------------------------------------------------------------------------------------
struct RbArgs {
    const double *u, *b, *uc;
    double *out;
    int nx, ny, nxc, nyc;
    long rs, crs;
    int ntx, yc, plainst;
    double a0, a2, a3, a4, a6, dinv, scale;
    const double *ctab, *dtab;
};

template <int NS, bool PRO, bool ZG, bool TAB>
__global__ void __launch_bounds__(256) k_rbgs_2d(const RbArgs a) {
    static_assert(NS == 2 || NS == 4, "one or two sweeps");
    static_assert(!(PRO && ZG), "the prolongation form reads u");
    using VT = V16<double>;
    constexpr int H = NS / 2, TP = 64 - 2 * H;                 // halo lanes a side; pairs a wave stores
    const int lane = threadIdx.x & 63;
    // (readfirstlane: the wave number, and with it every row index and row address below, lives on the scalar unit)
    const int wid = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int tx = wid % a.ntx, cy = wid / a.ntx;
    const int y0 = cy * a.yc, y1 = min(y0 + a.yc, a.ny);       // a.yc is even: every chunk starts on an even row
    if (y0 >= y1) return;                                      // whole wave
    const int pidx = tx * TP + lane - H;                       // pair index (= coarse column of the pair's odd fine column)
    const int x0 = 2 * pidx;
    const bool xin = (x0 >= 0 && x0 < a.nx);
    const bool lastvec = (x0 + 2 > a.nx);                      // the pair's second column is the ghost column (odd nx)
    const bool store = (lane >= H && lane < 64 - H && xin);
    const int xc = min(max(x0, 0), (a.nx - 1) & ~1);           // (even: 16-byte loads stay aligned whatever nx)
    const double *__restrict__ up_ = ZG ? nullptr : a.u + xc;
    const double *__restrict__ bp_ = a.b + xc;
    const double *__restrict__ cp_ = PRO ? a.uc + min(max(pidx, -1), a.nxc) : nullptr;
    const double *__restrict__ cm_ = PRO ? a.uc + min(max(pidx - 1, -1), a.nxc) : nullptr;
    double *__restrict__ op_ = a.out + x0;
    const VT Z = v16_zero<double>();
    const bool nts = a.plainst == 2 || (a.plainst == 0 && mgk_store_nt_2d(a.ny, a.rs));       // non-temporal stores: big fields only (mgk_dev.hpp)
    // a row of a field as it counts for a stage: zero outside the grid (rows -1 / ny and everything beyond, columns < 0 and >= nx)
    auto fix = [&](VT v, int y) -> VT {
        if (!xin || y < 0 || y >= a.ny) { v.v[0] = 0.0; v.v[1] = 0.0; }
        if (lastvec) v.v[1] = 0.0;
        return v;
    };
    auto ldraw = [&](int y) -> VT { return ZG ? Z : *reinterpret_cast<const VT *>(up_ + (long)min(max(y, -1), a.ny) * a.rs); };
    auto ldbraw = [&](int y) -> VT { return ldv_stream(bp_ + (long)min(max(y, 0), a.ny - 1) * a.rs, true); };
    // the parents of the fine row y: coarse rows pA(y) and pB(y) (the same row when y is odd), columns pidx - 1 and pidx
    struct C4 { double mA, cA, mB, cB; };
    auto pA = [&](int y) { return (y & 1) ? (y - 1) >> 1 : (y >> 1) - 1; };
    auto pB = [&](int y) { return (y & 1) ? (y - 1) >> 1 : (y >> 1); };
    auto ldc = [&](int y) -> C4 {
        C4 c = {0.0, 0.0, 0.0, 0.0};
        if (PRO) {
            const long ra = (long)min(max(pA(y), -1), a.nyc) * a.crs, rb = (long)min(max(pB(y), -1), a.nyc) * a.crs;
            c.mA = cm_[ra]; c.cA = cp_[ra]; c.mB = cm_[rb]; c.cB = cp_[rb];
        }
        return c;
    };
    // u + P uc on row y (terms in the order of the prolongation's row -- parents in ascending coarse index -- weights w = wi * wj, as k_jacobi3_2d)
    auto correct = [&](VT v, int y, const C4 &c) -> VT {
        if (PRO) {
            const bool two = ((y & 1) == 0);
            const double wi = two ? 0.5 : 1.0;
            const double wh = wi * 0.5, w1 = wi * 1.0;
            double s0 = 0.0, s1 = 0.0;
            s0 += wh * c.mA; s0 += wh * c.cA; s1 += w1 * c.cA;
            if (two) { s0 += wh * c.mB; s0 += wh * c.cB; s1 += w1 * c.cB; }
            v.v[0] = v.v[0] + s0; v.v[1] = v.v[1] + s1;
        }
        return fix(v, y);
    };
    // coefficients of grid row y: the launch constants, or row y of the tables (wave-uniform row index: scalar loads)
    struct K6 { double k0, k2, k3, k4, k6, kd; };
    auto ldk = [&](int y) -> K6 {
        K6 k = {a.a0, a.a2, a.a3, a.a4, a.a6, a.dinv};
        if (TAB) {
            const int yy_ = min(max(y, 0), a.ny - 1);
            const CDBL4 *cr_ = (const CDBL4 *)(a.ctab + 5 * (long)yy_);
            const CDBL4 *dr_ = (const CDBL4 *)(a.dtab + yy_);
            k.k0 = cr_[0]; k.k2 = cr_[1]; k.k3 = cr_[2]; k.k4 = cr_[3]; k.k6 = cr_[4]; k.kd = dr_[0];
        }
        return k;
    };
    // one stage on row y from the rows lo / c / hi of the field it starts from: element E of every pair is updated, the other one passes through
    auto stage = [&](auto ec, const VT &lo, const VT &c, const VT &hi, const VT &bb, int y, const K6 &kk) -> VT {
        constexpr int E = decltype(ec)::value;
        const double k0 = TAB ? kk.k0 : a.a0, k2 = TAB ? kk.k2 : a.a2, k3 = TAB ? kk.k3 : a.a3, k4 = TAB ? kk.k4 : a.a4, k6 = TAB ? kk.k6 : a.a6,
                     kd = TAB ? kk.kd : a.dinv;
        const double wv = (E == 0) ? lane_up<true>(c.v[1]) : c.v[0];
        const double ev = (E == 0) ? c.v[1] : lane_dn<true>(c.v[0]);
        double s = k0 * lo.v[E];
        s = s + k2 * wv;
        s = s + k3 * c.v[E];
        s = s + k4 * ev;
        s = s + k6 * hi.v[E];
        const double res = bb.v[E] - s;
        const double zz = res * kd;
        VT o = c;
        o.v[E] = c.v[E] + a.scale * zz;
        return fix(o, y);
    };
    auto put = [&](const VT &o, int y) {
        if (store) {
            if (lastvec) op_[(long)y * a.rs] = o.v[0];       // (the ghost column is never written)
            else stv_policy(op_ + (long)y * a.rs, o, nts);
        }
    };
    // the rings: phase K = (t - t0) mod NS.  u: ua = UU[K & 1] (row t+NS-2), ub = UU[(K+1) & 1] (row t+NS-1); b: row t+j = BB[(K+j) % NS];
    // stage q (1 .. NS-1): RR[q-1][K & 1] is its row t+NS-q-2, RR[q-1][(K+1) & 1] its row t+NS-q-1
    VT UU[2] = {Z, Z};
    VT BB[NS];
    VT RR[NS - 1][2];
#pragma unroll
    for (int q = 0; q < NS; q++) BB[q] = Z;
#pragma unroll
    for (int q = 0; q < NS - 1; q++) { RR[q][0] = Z; RR[q][1] = Z; }
    // one marching step: ur = the raw row t+NS of u with its parents pc, bnext = the raw row t+NS of b
    auto step = [&](auto kc, int t, const VT &ur, const C4 &pc, const VT &bnext) {
        constexpr int K = decltype(kc)::value;
        typedef std::integral_constant<int, (K + 1) & 1> EC;      // t0 is even: every stage of this step updates element (t + 1) & 1
        VT &ua = UU[K & 1], &ub = UU[(K + 1) & 1];
        const VT uc = ZG ? Z : correct(ur, t + NS, pc);
        const VT f1 = stage(EC{}, ua, ub, uc, BB[(K + NS - 1) % NS], t + NS - 1, ldk(t + NS - 1));
        ua = uc;                                                  // (the next phase's ub)
        if constexpr (NS == 2) {
            if (t >= y0) put(stage(EC{}, RR[0][K & 1], RR[0][(K + 1) & 1], f1, BB[K % NS], t, ldk(t)), t);
        } else {
            if (t >= y0 - 4) {                                    // wave-uniform, as the two below
                const VT f2 = stage(EC{}, RR[0][K & 1], RR[0][(K + 1) & 1], f1, BB[(K + 2) % NS], t + 2, ldk(t + 2));
                if (t >= y0 - 2) {
                    const VT f3 = stage(EC{}, RR[1][K & 1], RR[1][(K + 1) & 1], f2, BB[(K + 1) % NS], t + 1, ldk(t + 1));
                    if (t >= y0) put(stage(EC{}, RR[2][K & 1], RR[2][(K + 1) & 1], f3, BB[K % NS], t, ldk(t)), t);
                    RR[2][K & 1] = f3;
                }
                RR[1][K & 1] = f2;
            }
        }
        RR[0][K & 1] = f1;
        BB[K % NS] = fix(bnext, t + NS);                          // (the next phase's row t + NS - 1)
    };
    const int t0 = y0 - 2 * NS + 2;
    VT UR[2] = {Z, Z}, BN[2];                                     // the loads a step consumes are requested a step ahead: two sets, roles by phase
    C4 PC[2];
    UU[0] = correct(ldraw(t0 + NS - 2), t0 + NS - 2, ldc(t0 + NS - 2));
    UU[1] = correct(ldraw(t0 + NS - 1), t0 + NS - 1, ldc(t0 + NS - 1));
    UR[0] = ldraw(t0 + NS);
    PC[0] = ldc(t0 + NS);
    PC[1] = PC[0];
    BB[NS - 1] = fix(ldbraw(t0 + NS - 1), t0 + NS - 1);
    BN[0] = ldbraw(t0 + NS);
    auto S = [&](auto kc, int t) {
        constexpr int K = decltype(kc)::value;
        UR[(K + 1) & 1] = ldraw(t + NS + 1);
        PC[(K + 1) & 1] = ldc(t + NS + 1);
        BN[(K + 1) & 1] = ldbraw(t + NS + 1);
        step(kc, t, UR[K & 1], PC[K & 1], BN[K & 1]);
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2 % NS> I2;
    typedef std::integral_constant<int, 3 % NS> I3;
    int t = t0;
    if constexpr (NS == 2) {
        for (; t + 2 <= y1; t += 2) { S(I0{}, t); S(I1{}, t + 1); }
        if (t < y1) S(I0{}, t);
    } else {
        for (; t + 4 <= y1; t += 4) { S(I0{}, t); S(I1{}, t + 1); S(I2{}, t + 2); S(I3{}, t + 3); }
        if (t < y1) { S(I0{}, t); t++; }
        if (t < y1) { S(I1{}, t); t++; }
        if (t < y1) { S(I2{}, t); t++; }
    }
}
MGK_PRELOAD_UNIT(k_rbgs_2d<4, false, false, false>)

// shapes: any 2-D grid
template <bool PRO>
static int rbgs_2d(mgk_ctx *c, const mgk_geom *g, const mgk_geom *gc, const double *coef, double dinv, double scale, const double *ctab, const double *dtab,
                   int nsweeps, const double *b, const double *uc, const double *u, double *unew, void *stream) {
    const char *name = PRO ? "mgk_prolong_rbgs_2d_f64: bad arguments" : "mgk_rbgs_2d_f64: bad arguments";
    if (!c || !g || g->dim != 2 || g->nx < 1 || g->ny < 1 || (!coef && !ctab) || (ctab && !dtab) || !b || !unew || unew == u || unew == b || (PRO && !u))
        return fail(MGK_EINVAL, name);
    if (nsweeps != 1 && nsweeps != 2) return fail(MGK_EINVAL, PRO ? "mgk_prolong_rbgs_2d_f64: nsweeps must be 1 or 2" : "mgk_rbgs_2d_f64: nsweeps must be 1 or 2");
    RbArgs a; memset(&a, 0, sizeof(a));
    a.u = u ? u + g->org : nullptr; a.b = b + g->org; a.out = unew + g->org;
    a.nx = g->nx; a.ny = g->ny; a.rs = g->pitch;
    if (PRO) {
        if (!gc || !uc || gc->dim != 2 || g->nx != 2 * gc->nx + 1 || g->ny != 2 * gc->ny + 1) return fail(MGK_EINVAL, "mgk_prolong_rbgs_2d_f64: coarse grid does not match");
        a.uc = uc + gc->org; a.nxc = gc->nx; a.nyc = gc->ny; a.crs = gc->pitch;
    }
    if (coef) { a.a0 = coef[0]; a.a2 = coef[1]; a.a3 = coef[2]; a.a4 = coef[3]; a.a6 = coef[4]; }
    a.dinv = dinv; a.scale = scale; a.ctab = ctab; a.dtab = dtab;
    const int tp = 64 - 2 * nsweeps;                          // pairs a wave stores
    a.ntx = ((g->nx + 1) / 2 + tp - 1) / tp;
    // ~4096 waves (16 per CU) marching over chunks of at least 12 rows, an EVEN number (the kernel's colours are constants of the phase);
    // the second knob of mgk_set_tuning gives the chunk length (rounded up to even)
    a.yc = cut_chunks(c, g->ny, a.ntx, 4096, {/*min*/ 12, true, /*even*/ true, /*clamp*/ false, /*hint*/ 0, 0}).len;
    const long waves = (long)a.ntx * ((g->ny + a.yc - 1) / a.yc);
    const unsigned nblk = (unsigned)((waves + 3) / 4);
    const int sp = store_policy();
    a.plainst = sp == 0 ? 1 : sp == 1 ? 2 : 0;                // default: by field size (mgk_store_nt_2d)
    hipStream_t st = S(c, stream);
#define RB_LAUNCH(NSV, ZGV, TABV) hipLaunchKernelGGL((k_rbgs_2d<NSV, PRO, ZGV, TABV>), dim3(nblk), dim3(256), 0, st, a)
#define RB_LAUNCH_ZT(NSV)                                                                 \
    do {                                                                                  \
        if constexpr (PRO) { if (ctab) RB_LAUNCH(NSV, false, true); else RB_LAUNCH(NSV, false, false); } \
        else if (!u) { if (ctab) RB_LAUNCH(NSV, true, true); else RB_LAUNCH(NSV, true, false); }        \
        else { if (ctab) RB_LAUNCH(NSV, false, true); else RB_LAUNCH(NSV, false, false); }              \
    } while (0)
    if (nsweeps == 1) RB_LAUNCH_ZT(2); else RB_LAUNCH_ZT(4);
#undef RB_LAUNCH_ZT
#undef RB_LAUNCH
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int mgk_rbgs_2d_f64(mgk_ctx *c, const mgk_geom *g, const double *coef, double dinv, double scale, const double *ctab, const double *dtab,
                               int nsweeps, const double *b, const double *u, double *unew, void *stream) {
    return rbgs_2d<false>(c, g, nullptr, coef, dinv, scale, ctab, dtab, nsweeps, b, nullptr, u, unew, stream);
}
extern "C" int mgk_prolong_rbgs_2d_f64(mgk_ctx *c, const mgk_geom *gf, const mgk_geom *gc, const double *coef, double dinv, double scale,
                                       const double *ctab, const double *dtab, int nsweeps, const double *b, const double *uc, const double *u,
                                       double *unew, void *stream) {
    return rbgs_2d<true>(c, gf, gc, coef, dinv, scale, ctab, dtab, nsweeps, b, uc, u, unew, stream);
}
