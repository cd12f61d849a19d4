/* san_cheby.c -- a Chebyshev solve and a fixed run of cycles through mg_solver.c + mg_cheby.c over the host-memory stand-ins
 * (tests/mock_mgk_cheby.cpp), as a plain executable so that it can be built with -fsanitize=address,undefined
 * (tests/test_cheby_fused_cpu.py).  argv: dim npts levels mesh fuse ncycles outfile.  Writes: iterations of the solve, its residual
 * history and solution, then the history and solution after reset + ncycles cycles, and the stand-ins' execution counts, as text
 * (%.17g round-trips a double). */
#include <stdio.h>
#include <stdlib.h>
#include "mgsolve.h"

int mock_cheby_calls(int which);
void mock_cheby_calls_reset(void);

#define OK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: rc=%d: %s\n", #call, rc_, mg_last_error()); return 2; } } while (0)

static void dump(FILE *f, mg_solver *s, const char *tag, double *u, long n) {
    const int it = mg_solver_iterations(s);
    const double *rn = mg_solver_rnorm(s);
    fprintf(f, "%s_iters %d\n%s_rnorm", tag, it, tag);
    for (int q = 0; q <= it; q++) fprintf(f, " %.17g", rn[q]);
    fprintf(f, "\n%s_calls", tag);
    for (int q = 0; q < 5; q++) fprintf(f, " %d", mock_cheby_calls(q));
    fprintf(f, "\n%s_u", tag);
    for (long q = 0; q < n; q++) fprintf(f, " %.17g", u[q]);
    fprintf(f, "\n");
}

int main(int argc, char **argv) {
    if (argc != 8) { fprintf(stderr, "usage: san_cheby dim npts levels mesh fuse ncycles outfile\n"); return 1; }
    mg_config c;
    mg_config_default(&c);
    c.dim = atoi(argv[1]); c.npts = atoi(argv[2]); c.levels = atoi(argv[3]); c.mesh = atoi(argv[4]); c.fuse = atoi(argv[5]);
    const int ncycles = atoi(argv[6]);
    c.v[0] = 3; c.v[1] = 3; c.maxiter = 60;
    c.ksp_type = MG_KSP_CHEBYSHEV; c.emin = 0.2; c.emax = 2.0;
    mg_solver *s = NULL;
    OK(mg_solver_create(&s, &c, NULL));
    OK(mg_solver_set_rhs_problem(s));
    const long n = mg_solver_local_unknowns(s);
    double *u = (double *)malloc(sizeof(double) * (size_t)n);
    FILE *f = fopen(argv[7], "w");
    if (!u || !f) return 3;
    mock_cheby_calls_reset();
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "solve", u, n);
    mock_cheby_calls_reset();
    OK(mg_solver_reset(s));
    OK(mg_solver_cycles(s, ncycles));
    OK(mg_solver_sync(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "cycles", u, n);
    fclose(f);
    free(u);
    mg_solver_destroy(s);
    return 0;
}
