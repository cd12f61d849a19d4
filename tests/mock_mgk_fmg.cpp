// mock_mgk_fmg.cpp -- host-memory stand-ins for the four full-multigrid entry points (mgk_interp_jacobi2_ok_f64, mgk_interp_jacobi2_f64,
// mgk_interp_jacobi3_2d_f64, mgk_tail_fmg_f64) in the canonical arithmetic of tests/mock_mgk.cpp, built from that file's helpers (corrected,
// st_op, j3_sweeps, restrict_fw, prolong_at), so that csrc/mg_fmg.c -- its buffer roles, pre_done, the flag resets after the stages -- runs on
// the CPU tier (tests/test_random_sessions_cpu.py, tools/stress_sessions_mock.py).  tests/mock_mgk_gmres.cpp is included textually and stays as
// it is (and through it mock_mgk.cpp): one library then serves solve, cycles, fmg, solve_fmg and solve_gmres on the same handle.
// "0 + P uc" adds to a literal zeroed field, as mgk_prolong_add_f64 on zeros does (0 + (-0) = +0).  Recorded when a graph is being captured,
// like the other stand-ins.  Every stand-in counts its calls.  TEST INFRASTRUCTURE ONLY: no product source names this file.
#include "mock_mgk_gmres.cpp"

static int g_fmg_calls[3] = {0, 0, 0};              // interp_jacobi2, interp_jacobi3_2d, tail_fmg
extern "C" int mock_fmg_calls(int which) { return (which >= 0 && which < 3) ? g_fmg_calls[which] : -1; }
extern "C" void mock_fmg_calls_reset(void) { g_fmg_calls[0] = g_fmg_calls[1] = g_fmg_calls[2] = 0; }

extern "C" {
int mgk_interp_jacobi2_ok_f64(const mgk_geom *gf, const mgk_geom *gc) { return mgk_prolong_jacobi2_ok_f64(gf, gc); }
// unew = J(J(0 + P uc)); the old unew is never read
int mgk_interp_jacobi2_f64(mgk_ctx *c, const mgk_geom *gf, const mgk_geom *gc, const double *coef, double dinv, double scale, const double *b, const double *uc, double *o, void *) {
    if (!c || !coef || !b || !uc || !o || o == b || o == uc || !mgk_interp_jacobi2_ok_f64(gf, gc)) return fail(MGK_EINVAL, "mgk_interp_jacobi2_f64");
    g_fmg_calls[0]++;
    const mgk_geom F = *gf, Cg = *gc; std::vector<double> k(coef, coef + 7);
    return run(c, [=] {
        std::vector<double> z(F.total, 0.0), w(F.total, 0.0);
        std::vector<double> t = corrected<double>(F, Cg, uc, z.data());
        st_op<double>(M_JACOBI, F, k.data(), dinv, scale, 0, 0, 0, b, t.data(), (const double *)nullptr, w.data(), 0, F.nz);
        st_op<double>(M_JACOBI, F, k.data(), dinv, scale, 0, 0, 0, b, w.data(), (const double *)nullptr, o, 0, F.nz);
    });
}
// unew = J(J(J(0 + P uc))), 2-D, any grid
int mgk_interp_jacobi3_2d_f64(mgk_ctx *c, const mgk_geom *gf, const mgk_geom *gc, const double *coef, double dinv, double scale, const double *b, const double *uc, double *o, void *) {
    if (!c || !coef || !b || !uc || !o || o == b || o == uc || !xfer_ok(gf, gc) || gf->dim != 2) return fail(MGK_EINVAL, "mgk_interp_jacobi3_2d_f64");
    g_fmg_calls[1]++;
    const mgk_geom F = *gf, Cg = *gc; std::vector<double> k(coef, coef + 7);
    return run(c, [=] {
        std::vector<double> z(F.total, 0.0);
        std::vector<double> t = corrected<double>(F, Cg, uc, z.data());
        j3_sweeps(F, k.data(), dinv, scale, nullptr, nullptr, b, t.data(), o, 3);
    });
}
// FMG(nu) on the levels of the tail (include/mgk.h): b_l = R b_{l-1} down the levels, v1 sweeps from the zero guess on the last one, then for
// r from the second-coarsest level up: u_r = 0 + P u_{r+1} and nu cycles rooted at r -- v0 sweeps on r from that guess, below r the cycle of
// tail_api (residual + full weighting + sweeps from zero down, v1 on the last level; prolongation + v0 sweeps up)
int mgk_tail_fmg_f64(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, const double *coef7, const double *dinv, double scale, int v0, int v1, int nu,
                     const double *b, double *u, void *) {
    if (!c || !g0 || !n || !coef7 || !dinv || !b || !u || b == u || nlev < 2 || nlev > 8 || nu < 1 || v0 < 0 || v1 < 0 || n[0] != g0->nx || n[0] > mgk_tail_max_n(g0->dim))
        return fail(MGK_EINVAL, "mgk_tail_fmg_f64");
    for (int l = 1; l < nlev; l++) if (n[l - 1] != 2 * n[l] + 1) return fail(MGK_EINVAL, "mgk_tail_fmg_f64: hierarchy");
    g_fmg_calls[2]++;
    const mgk_geom G0 = *g0; std::vector<int> nn(n, n + nlev);
    std::vector<double> k7(coef7, coef7 + 7 * nlev), di(dinv, dinv + nlev);
    return run(c, [=] {
        std::vector<mgk_geom> G(nlev);
        std::vector<std::vector<double>> U(nlev), W(nlev), B(nlev);
        for (int l = 0; l < nlev; l++) {
            mgk_geom_init(&G[l], G0.dim, nn[l], nn[l], nn[l]);
            U[l].assign(G[l].total, 0.0); W[l].assign(G[l].total, 0.0); B[l].assign(G[l].total, 0.0);
        }
        memcpy(B[0].data(), b, sizeof(double) * (size_t)G0.total);
        auto smooth = [&](int l, int sweeps, bool zero) {
            for (int it = 0; it < sweeps; it++) {
                if (it == 0 && zero) {
                    std::fill(W[l].begin(), W[l].end(), 0.0);
                    for (int k = 0; k < G[l].nz; k++) for (int i = 0; i < G[l].ny; i++) for (int j = 0; j < G[l].nx; j++) {
                        const double zx = at(B[l].data(), G[l], k, i, j) * di[l]; at(W[l].data(), G[l], k, i, j) = scale * zx; }
                } else st_op<double>(M_JACOBI, G[l], &k7[7 * l], di[l], scale, 0, 0, 0, B[l].data(), U[l].data(), (const double *)nullptr, W[l].data(), 0, NMARCH(&G[l]));
                U[l].swap(W[l]);
            }
        };
        auto down = [&](int l) {                        // b_l = R (b_{l-1} - A u_{l-1}): the FMG right-hand side of level l is spent by then
            st_op<double>(M_RESIDUAL, G[l - 1], &k7[7 * (l - 1)], 1, 1, 0, 0, 0, B[l - 1].data(), U[l - 1].data(), (const double *)nullptr, W[l - 1].data(), 0, NMARCH(&G[l - 1]));
            restrict_fw<double>(G[l - 1], G[l], W[l - 1].data(), B[l].data(), 0, G[l].dim == 3 ? G[l].nz : 1);
        };
        auto prolong_add = [&](int l) {                 // u_l += P u_{l+1}
            for (int k = 0; k < (G[l].dim == 3 ? G[l].nz : 1); k++) for (int i = 0; i < G[l].ny; i++) for (int j = 0; j < G[l].nx; j++)
                at(U[l].data(), G[l], k, i, j) = at(U[l].data(), G[l], k, i, j) + prolong_at(G[l], G[l + 1], U[l + 1].data(), G[l].dim == 3 ? k : 1, i, j);
        };
        for (int l = 1; l < nlev; l++) restrict_fw<double>(G[l - 1], G[l], B[l - 1].data(), B[l].data(), 0, G[l].dim == 3 ? G[l].nz : 1);
        std::fill(U[nlev - 1].begin(), U[nlev - 1].end(), 0.0);
        smooth(nlev - 1, v1, true);
        for (int r = nlev - 2; r >= 0; r--) {
            std::fill(U[r].begin(), U[r].end(), 0.0);
            prolong_add(r);
            for (int q = 0; q < nu; q++) {
                smooth(r, v0, false);
                for (int l = r + 1; l < nlev; l++) {
                    down(l);
                    std::fill(U[l].begin(), U[l].end(), 0.0);
                    smooth(l, l == nlev - 1 ? v1 : v0, true);
                }
                for (int l = nlev - 2; l >= r; l--) { prolong_add(l); smooth(l, v0, false); }
            }
        }
        for (int k = 0; k < (G0.dim == 3 ? G0.nz : 1); k++) for (int i = 0; i < G0.ny; i++) memcpy(&at(u, G0, k, i, 0), &at(U[0].data(), G[0], k, i, 0), sizeof(double) * (size_t)G0.nx);
    });
}
}   // extern "C"
