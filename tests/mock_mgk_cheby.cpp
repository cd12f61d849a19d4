// mock_mgk_cheby.cpp -- host-memory stand-ins for the Chebyshev entry points of the fused cycle (mgk_cheby3_2d_f64 / _sumsq / _zero,
// mgk_prolong_cheby3_2d_f64, mgk_tail_cycle_cheby_f64) in the canonical arithmetic: compositions of the single sweep and the single
// recurrence step of mock_mgk.cpp.  That file's context, its run() (which records into a capture), st_op<> and deliver() are private to
// it, so it is included textually (and stays as it is): the stand-ins here record and replay like the others.  Linked with mg_solver.c,
// mg_comm.c and mg_cheby.c by tests/test_cheby_fused_cpu.py.  Every stand-in counts its EXECUTIONS (a replayed graph counts again).
#include "mock_mgk.cpp"
#include <array>
#include "mg_cheby_coefs.h"

static int g_cheby_calls[5] = {0, 0, 0, 0, 0};      // plain, sumsq, zero, prolong, tail
extern "C" int mock_cheby_calls(int which) { return (which >= 0 && which < 5) ? g_cheby_calls[which] : -1; }
extern "C" void mock_cheby_calls_reset(void) { for (int q = 0; q < 5; q++) g_cheby_calls[q] = 0; }

// KSPSolve(KSPCHEBYSHEV, max_it = 3) from the field `first` (zero: from the zero guess, `first` is not read), result into o
static void cheby3_steps(const mgk_geom &G, const double *coef, double dinv, const std::array<double, 7> &c7, const double *ctab, const double *dtab,
                         const double *b, const double *first, bool zero, double *o) {
    std::vector<double> z(G.total, 0.0), p1(G.total, 0.0), p2(G.total, 0.0);
    const double *k = ctab ? nullptr : coef;
    const double di = ctab ? 1.0 : dinv;
    const double *p0 = zero ? z.data() : first;
    if (zero) {
        for (int i = 0; i < G.ny; i++) for (int j = 0; j < G.nx; j++) { const double zx = at(b, G, 0, i, j) * (dtab ? dtab[i] : dinv); at(p1.data(), G, 0, i, j) = c7[0] * zx; }
    } else st_op<double>(M_JACOBI, G, k, di, c7[0], 0, 0, 0, b, p0, (const double *)nullptr, p1.data(), 0, G.ny, ctab, dtab);
    st_op<double>(M_CHEBY, G, k, di, 1, c7[1], c7[2], c7[3], b, p1.data(), p0, p2.data(), 0, G.ny, ctab, dtab);
    st_op<double>(M_CHEBY, G, k, di, 1, c7[4], c7[5], c7[6], b, p2.data(), p1.data(), o, 0, G.ny, ctab, dtab);
}
static std::array<double, 7> arr7(const double *c) { std::array<double, 7> a; for (int q = 0; q < 7; q++) a[q] = c[q]; return a; }

extern "C" {
int mgk_cheby3_2d_f64(mgk_ctx *c, const mgk_geom *g, const double *coef, double dinv, const double *cheb, const double *ctab, const double *dtab,
                      const double *b, const double *u, double *o, void *) {
    if (!c || !g || g->dim != 2 || !cheb || (!coef && !ctab) || (ctab && !dtab) || !b || !u || !o || u == o || b == o) return fail(MGK_EINVAL, "mgk_cheby3_2d_f64");
    const mgk_geom G = *g; std::vector<double> k(7, 0.0); if (coef) k.assign(coef, coef + 7);
    const std::array<double, 7> c7 = arr7(cheb);
    return run(c, [=] { g_cheby_calls[0]++; cheby3_steps(G, k.data(), dinv, c7, ctab, dtab, b, u, false, o); });
}
int mgk_cheby3_2d_sumsq_f64(mgk_ctx *c, const mgk_geom *g, const double *coef, double dinv, const double *cheb, const double *ctab, const double *dtab,
                            const double *b, const double *u, double *o, double *out, void *) {
    if (!c || !g || g->dim != 2 || !cheb || (!coef && !ctab) || (ctab && !dtab) || !b || !u || !o || u == o || b == o || !out) return fail(MGK_EINVAL, "mgk_cheby3_2d_sumsq_f64");
    if (c->capturing) return fail(MGK_EINVAL, "reduction to the host inside a capture");
    std::vector<double> r(g->total, 0.0);
    st_op<double>(M_RESIDUAL, *g, ctab ? nullptr : coef, 1, 1, 0, 0, 0, b, u, (const double *)nullptr, r.data(), 0, g->ny, ctab, (const double *)nullptr);
    g_cheby_calls[1]++;
    cheby3_steps(*g, coef, dinv, arr7(cheb), ctab, dtab, b, u, false, o);
    deliver(c, sumsq_field<double>(*g, r.data(), 0, g->ny), out);
    return 0;
}
int mgk_cheby3_2d_zero_f64(mgk_ctx *c, const mgk_geom *g, const double *coef, double dinv, const double *cheb, const double *ctab, const double *dtab,
                           const double *b, double *o, void *) {
    if (!c || !g || g->dim != 2 || !cheb || (!coef && !ctab) || (ctab && !dtab) || !b || !o || b == o) return fail(MGK_EINVAL, "mgk_cheby3_2d_zero_f64");
    const mgk_geom G = *g; std::vector<double> k(7, 0.0); if (coef) k.assign(coef, coef + 7);
    const std::array<double, 7> c7 = arr7(cheb);
    return run(c, [=] { g_cheby_calls[2]++; cheby3_steps(G, k.data(), dinv, c7, ctab, dtab, b, nullptr, true, o); });
}
int mgk_prolong_cheby3_2d_f64(mgk_ctx *c, const mgk_geom *gf, const mgk_geom *gc, const double *coef, double dinv, const double *cheb, const double *ctab,
                              const double *dtab, const double *b, const double *uc, const double *u, double *o, void *) {
    if (!c || !cheb || (!coef && !ctab) || (ctab && !dtab) || !b || !uc || !u || !o || u == o || b == o || !xfer_ok(gf, gc) || gf->dim != 2) return fail(MGK_EINVAL, "mgk_prolong_cheby3_2d_f64");
    const mgk_geom F = *gf, Cg = *gc; std::vector<double> k(7, 0.0); if (coef) k.assign(coef, coef + 7);
    const std::array<double, 7> c7 = arr7(cheb);
    return run(c, [=] { g_cheby_calls[3]++; std::vector<double> t = corrected<double>(F, Cg, uc, u); cheby3_steps(F, k.data(), dinv, c7, ctab, dtab, b, t.data(), false, o); });
}
// the tail levels of one cycle, every KSPSolve the restarted recurrence (the first step is always taken)
int mgk_tail_cycle_cheby_f64(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, const double *coef7, const double *dinv, const double *const *ctab,
                             const double *const *dtab, double emin, double emax, int v0, int v1, const double *b, double *u, void *) {
    typedef double T;
    if (!c || !g0 || !n || (!coef7 && !ctab) || (!dinv && !dtab) || !b || !u || nlev < 1 || nlev > 8 || n[0] != g0->nx || n[0] > mgk_tail_max_n(g0->dim) ||
        (ctab == nullptr) != (dtab == nullptr) || (ctab && g0->dim != 2) || v0 < 0 || v1 < 0 || v0 > 16 || v1 > 16 || !(emax > emin && emin > 0.0))
        return fail(MGK_EINVAL, "mgk_tail_cycle_cheby_f64");
    for (int l = 1; l < nlev; l++) if (n[l - 1] != 2 * n[l] + 1) return fail(MGK_EINVAL, "mgk_tail_cycle_cheby_f64: hierarchy");
    const mgk_geom G0 = *g0; std::vector<int> nn(n, n + nlev);
    std::vector<double> k7(7 * nlev, 0.0), di(nlev, 1.0);
    if (!ctab) { k7.assign(coef7, coef7 + 7 * nlev); di.assign(dinv, dinv + nlev); }
    std::vector<const double *> ct(nlev, nullptr), dt(nlev, nullptr);
    for (int l = 0; l < nlev && ctab; l++) { ct[l] = ctab[l]; dt[l] = dtab[l]; if (!ct[l] || !dt[l]) return fail(MGK_EINVAL, "mgk_tail_cycle_cheby_f64: null table"); }
    return run(c, [=] {
        g_cheby_calls[4]++;
        std::vector<mgk_geom> G(nlev);
        std::vector<std::vector<T>> U(nlev), W(nlev), P(nlev), B(nlev);
        for (int l = 0; l < nlev; l++) {
            mgk_geom_init(&G[l], G0.dim, nn[l], nn[l], nn[l]);
            U[l].assign(G[l].total, 0.0); W[l].assign(G[l].total, 0.0); P[l].assign(G[l].total, 0.0); B[l].assign(G[l].total, 0.0);
        }
        memcpy(B[0].data(), b, sizeof(T) * (size_t)G0.total);
        auto solve = [&](int l, int steps, bool zero) {         // U[l]: the guess in, the result out
            mg_cheby_rec rec;
            mg_cheby_begin(&rec, emin, emax);
            std::vector<T> &pkm1 = U[l], &pk = W[l], &pkp1 = P[l];
            if (zero) {
                std::fill(pkm1.begin(), pkm1.end(), 0.0); std::fill(pk.begin(), pk.end(), 0.0);
                for (int k = 0; k < G[l].nz; k++) for (int i = 0; i < G[l].ny; i++) for (int j = 0; j < G[l].nx; j++) {
                    const T zx = at(B[l].data(), G[l], k, i, j) * (dt[l] ? dt[l][i] : di[l]); at(pk.data(), G[l], k, i, j) = rec.scale * zx; }
            } else st_op<T>(M_JACOBI, G[l], &k7[7 * l], di[l], rec.scale, 0, 0, 0, B[l].data(), pkm1.data(), (const T *)nullptr, pk.data(), 0, NMARCH(&G[l]), ct[l], dt[l]);
            for (int it = 1; it < steps; it++) {
                double c3[3];
                mg_cheby_next(&rec, c3);
                std::fill(pkp1.begin(), pkp1.end(), 0.0);
                st_op<T>(M_CHEBY, G[l], &k7[7 * l], di[l], 1, c3[0], c3[1], c3[2], B[l].data(), pk.data(), pkm1.data(), pkp1.data(), 0, NMARCH(&G[l]), ct[l], dt[l]);
                pkm1.swap(pk); pk.swap(pkp1);                  // (pkm1, pk, pkp1) <- (pk, pkp1, pkm1)
            }
            U[l].swap(W[l]);                                    // the references: pk is W[l]
        };
        solve(0, nlev == 1 ? v1 : v0, true);
        for (int l = 1; l < nlev; l++) {
            st_op<T>(M_RESIDUAL, G[l - 1], &k7[7 * (l - 1)], 1, 1, 0, 0, 0, B[l - 1].data(), U[l - 1].data(), (const T *)nullptr, W[l - 1].data(), 0, NMARCH(&G[l - 1]), ct[l - 1], dt[l - 1]);
            restrict_fw<T>(G[l - 1], G[l], W[l - 1].data(), B[l].data(), 0, G[l].dim == 3 ? G[l].nz : 1);
            solve(l, l == nlev - 1 ? v1 : v0, true);
        }
        for (int l = nlev - 2; l >= 0; l--) {
            for (int k = 0; k < (G[l].dim == 3 ? G[l].nz : 1); k++) for (int i = 0; i < G[l].ny; i++) for (int j = 0; j < G[l].nx; j++)
                at(U[l].data(), G[l], k, i, j) = at(U[l].data(), G[l], k, i, j) + prolong_at(G[l], G[l + 1], U[l + 1].data(), G[l].dim == 3 ? k : 1, i, j);
            solve(l, v0, false);
        }
        for (int k = 0; k < (G0.dim == 3 ? G0.nz : 1); k++) for (int i = 0; i < G0.ny; i++) memcpy(&at(u, G0, k, i, 0), &at(U[0].data(), G[0], k, i, 0), sizeof(T) * (size_t)G0.nx);
    });
}
}   // extern "C"
