// tests/mock_mgk_faulty.cpp -- TEST INFRASTRUCTURE ONLY.  tests/mock_mgk.cpp plus five host functions with the signature of mgk_jacobi_f64: one
// right and four deliberately wrong in WHERE they store or WHAT they read, each in a way a comparison of interiors against a zero-filled or reused
// output buffer cannot see.  tests/test_guarded_cpu.py shows that tests/guarded.py passes the first and catches the other four.  Host loops over
// host memory inside the guard zones of that proxy: nothing faults.  Never built into anything under multigrid_petsc_amd/.
#include "mock_mgk.cpp"

static void faulty_sweep(const mgk_geom *g, const double *k, double d, double s, const double *b, const double *u, double *o, int zend) {
    st_op<double>(M_JACOBI, *g, k, d, s, 0, 0, 0, b, u, (const double *)nullptr, o, 0, zend);
}
#define FAULTY_ARGS mgk_ctx *c, const mgk_geom *g, const double *k, double d, double s, const double *b, const double *u, double *o, void *
#define FAULTY_CHECK if (!c || !g || !k || !b || !u || !o || u == o) return fail(MGK_EINVAL, "faulty_jacobi")

extern "C" {
// the sweep itself
int faulty_jacobi_right_f64(FAULTY_ARGS) { FAULTY_CHECK; faulty_sweep(g, k, d, s, b, u, o, NMARCH(g)); return 0; }
// a full-row store that puts the value of the last column into the right ghost column j = nx of the last row
int faulty_jacobi_ghost_column_f64(FAULTY_ARGS) {
    FAULTY_CHECK;
    faulty_sweep(g, k, d, s, b, u, o, NMARCH(g));
    at(o, *g, g->dim == 3 ? g->nz - 1 : 0, g->ny - 1, g->nx) = at(o, *g, g->dim == 3 ? g->nz - 1 : 0, g->ny - 1, g->nx - 1);
    return 0;
}
// a row "beyond the ghost row" that is one element too long: a store at offset g->total
int faulty_jacobi_past_the_end_f64(FAULTY_ARGS) { FAULTY_CHECK; faulty_sweep(g, k, d, s, b, u, o, NMARCH(g)); o[g->total] = 1.0; return 0; }
// the last interior row (3-D: of the last plane) is never written
int faulty_jacobi_skips_last_row_f64(FAULTY_ARGS) {
    FAULTY_CHECK;
    std::vector<double> keep((size_t)g->nx);
    const int kl = g->dim == 3 ? g->nz - 1 : 0;
    for (int j = 0; j < g->nx; j++) keep[(size_t)j] = at(o, *g, kl, g->ny - 1, j);
    faulty_sweep(g, k, d, s, b, u, o, NMARCH(g));
    for (int j = 0; j < g->nx; j++) at(o, *g, kl, g->ny - 1, j) = keep[(size_t)j];
    return 0;
}
// the old content of unew is added into the result (an accumulating store where a plain one belongs)
int faulty_jacobi_adds_old_output_f64(FAULTY_ARGS) {
    FAULTY_CHECK;
    std::vector<double> old((size_t)g->total);
    memcpy(old.data(), o, sizeof(double) * (size_t)g->total);
    faulty_sweep(g, k, d, s, b, u, o, NMARCH(g));
    for (int kk = 0; kk < (g->dim == 3 ? g->nz : 1); kk++)
        for (int i = 0; i < g->ny; i++)
            for (int j = 0; j < g->nx; j++) at(o, *g, kk, i, j) = at(old.data(), *g, kk, i, j) + at(o, *g, kk, i, j);
    return 0;
}
}   // extern "C"
