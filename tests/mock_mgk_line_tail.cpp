// mock_mgk_line_tail.cpp -- host-memory stand-in for mgk_tail_cycle_line_f64 (include/mgk.h): the levels of a line cycle that the product runs
// in one launch, built from the stand-ins' own per-pass functions -- the y and x line passes of tests/mock_mgk_line.cpp /
// tests/mock_mgk_xline.cpp, the row-table residual, the restriction and the prolongation of tests/mock_mgk.cpp -- in the order of the
// launch-by-launch loop, on fields of its own.  tests/mock_mgk_xline.cpp (and with it the other two) is included textually and stays as it is.
// Linked with mg_solver.c, mg_comm.c, mg_line.c, mg_xline.c and mg_line_tail.c by tests/test_line_tail_cpu.py.  The log of line passes gets
// ONE letter per executed tail call, 'T'; the passes made inside it are not logged, so a line pass of a tail level made by launch would show.
#include "mock_mgk_xline.cpp"
#include <vector>

static int g_line_tail_calls = 0;
extern "C" int mock_line_tail_calls(void) { return g_line_tail_calls; }

extern "C" int mgk_tail_cycle_line_f64(mgk_ctx *c, const mgk_geom *g0, int nlev, const int *n, int pc, const double *const *ctab,
                                       const double *const *ltab, const double *const *gtab, const double *const *qtab,
                                       const double *const *xgtab, const long *xgs, double scale, int v0, int v1, const double *b, double *u, void *) {
    if (!c || !g0 || !n || !ctab || !b || !u || nlev < 1 || nlev > 8 || v0 < 0 || v1 < 0 || pc < 1 || pc > 3 || g0->dim != 2 ||
        n[0] != g0->nx || g0->ny != g0->nx || n[0] > mgk_tail_max_n(2))
        return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64");
    const bool ysw = pc != 2, xsw = pc != 1;
    if ((ysw && (!ltab || !gtab || !qtab)) || (xsw && (!xgtab || !xgs))) return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: null tables");
    std::vector<int> nn(n, n + nlev);
    std::vector<const double *> ct(nlev), lt(nlev, nullptr), gt(nlev, nullptr), qt(nlev, nullptr), xg(nlev, nullptr);
    std::vector<long> xs(nlev, 0);
    for (int l = 0; l < nlev; l++) {
        if (l > 0 && n[l - 1] != 2 * n[l] + 1) return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: hierarchy");
        ct[l] = ctab[l];
        if (ysw) { lt[l] = ltab[l]; gt[l] = gtab[l]; qt[l] = qtab[l]; }
        if (xsw) { xg[l] = xgtab[l]; xs[l] = xgs[l]; }
        if (!ct[l] || (ysw && (!lt[l] || !gt[l] || !qt[l])) || (xsw && (!xg[l] || (xs[l] != 0 && xs[l] < n[l])))) return fail(MGK_EINVAL, "mgk_tail_cycle_line_f64: table");
    }
    const mgk_geom G0 = *g0;
    return run(c, [=] {
        // the passes below execute at once (a recorded graph is being replayed, or nothing is being captured); what they log is taken back
        note_y();
        const size_t mark = g_xline_log.size();
        const int calls[2] = {g_line_calls[0], g_line_calls[1]};
        std::vector<mgk_geom> G(nlev);
        std::vector<std::vector<double>> U(nlev), Z(nlev), B(nlev);
        for (int l = 0; l < nlev; l++) {
            mgk_geom_init(&G[l], 2, nn[l], nn[l], 1);
            U[l].assign(G[l].total, 0.0); Z[l].assign(G[l].total, 0.0); B[l].assign(G[l].total, 0.0);
        }
        for (int i = 0; i < G0.ny; i++) for (int j = 0; j < G0.nx; j++) at(B[0].data(), G[0], 0, i, j) = at(b, G0, 0, i, j);
        auto smooth = [&](int l, int sweeps, bool zero) {            // KSPSolve, max_it = sweeps; with no sweep from the zero guess U stays 0
            for (int k = 0; k < sweeps; k++) {
                const double *uin = (zero && k == 0) ? nullptr : U[l].data();
                if (pc == 2 || (pc == 3 && (k & 1))) {
                    mgk_xline_forward_f64(c, &G[l], ct[l], xg[l], xs[l], B[l].data(), uin, Z[l].data(), nullptr);
                    mgk_xline_backward_f64(c, &G[l], ct[l], xg[l], xs[l], scale, Z[l].data(), uin, U[l].data(), nullptr);
                } else {
                    mgk_line_forward_f64(c, &G[l], ct[l], lt[l], gt[l], B[l].data(), uin, Z[l].data(), nullptr);
                    mgk_line_backward_f64(c, &G[l], qt[l], scale, Z[l].data(), uin, U[l].data(), nullptr);
                }
            }
        };
        smooth(0, nlev == 1 ? v1 : v0, true);
        for (int l = 1; l < nlev; l++) {
            mgk_rowcoef_f64(c, &G[l - 1], 1, ct[l - 1], nullptr, 1.0, B[l - 1].data(), U[l - 1].data(), Z[l - 1].data(), nullptr);
            mgk_restrict_fw_f64(c, &G[l - 1], &G[l], Z[l - 1].data(), B[l].data(), nullptr);
            smooth(l, l == nlev - 1 ? v1 : v0, true);
        }
        for (int l = nlev - 2; l >= 0; l--) {
            mgk_prolong_add_f64(c, &G[l], &G[l + 1], U[l + 1].data(), U[l].data(), nullptr);
            smooth(l, v0, false);
        }
        for (int i = 0; i < G0.ny; i++) for (int j = 0; j < G0.nx; j++) at(u, G0, 0, i, j) = at(U[0].data(), G[0], 0, i, j);
        g_line_calls[0] = calls[0]; g_line_calls[1] = calls[1];
        g_seen[0] = calls[0]; g_seen[1] = calls[1];
        g_xline_log.resize(mark);
        g_xline_log += 'T';
        g_line_tail_calls++;
    });
}
