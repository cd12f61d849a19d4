/* san_gmres.c -- GMRES solves through mg_solver.c + mg_gmres.c over the host-memory stand-ins (tests/mock_mgk_gmres.cpp), as a plain
 * executable so that it can be built with -fsanitize=address,undefined (tests/test_gmres_cpu.py).
 * argv: dim npts levels mesh scale restart maxiter rhsfile outfile (rhsfile: raw doubles of the compact right-hand side, "-" = the
 * manufactured one).  Runs solve_gmres, again, with another restart length, then reset + solve; checks the refusals (restart out of range;
 * more than one rank, through the private header: gmres_check reads the configuration alone); writes the histories and fields as text
 * (%.17g round-trips a double). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mg_solver_internal.h"

#define OK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: rc=%d: %s\n", #call, rc_, mg_last_error()); return 2; } } while (0)
#define REFUSED(call, msg) do { int rc_ = (call); if (rc_ != MGK_EINVAL || !strstr(mg_last_error(), msg)) { \
    fprintf(stderr, "%s: rc=%d: %s (expected a refusal with '%s')\n", #call, rc_, mg_last_error(), msg); return 4; } } while (0)

static void dump(FILE *f, mg_solver *s, const char *tag, const double *u, long n) {
    const int it = mg_solver_iterations(s);
    const double *rn = mg_solver_rnorm(s);
    fprintf(f, "%s_iters %d\n%s_rnorm", tag, it, tag);
    for (int q = 0; q <= it; q++) fprintf(f, " %.17g", rn[q]);
    fprintf(f, "\n%s_u", tag);
    for (long q = 0; q < n; q++) fprintf(f, " %.17g", u[q]);
    fprintf(f, "\n");
}

int main(int argc, char **argv) {
    if (argc != 10) { fprintf(stderr, "usage: san_gmres dim npts levels mesh scale restart maxiter rhsfile outfile\n"); return 1; }
    mg_config c;
    mg_config_default(&c);
    c.dim = atoi(argv[1]); c.npts = atoi(argv[2]); c.levels = atoi(argv[3]); c.mesh = atoi(argv[4]); c.scale = atof(argv[5]);
    const int restart = atoi(argv[6]);
    c.maxiter = atoi(argv[7]);
    c.v[0] = 3; c.v[1] = 3;
    mg_solver *s = NULL;
    OK(mg_solver_create(&s, &c, NULL));
    const long n = mg_solver_local_unknowns(s);
    double *u = (double *)malloc(sizeof(double) * (size_t)n), *u2 = (double *)malloc(sizeof(double) * (size_t)n);
    FILE *f = fopen(argv[9], "w");
    if (!u || !u2 || !f) return 3;
    if (strcmp(argv[8], "-")) {
        FILE *r = fopen(argv[8], "rb");
        if (!r || fread(u, sizeof(double), (size_t)n, r) != (size_t)n) return 3;
        fclose(r);
        OK(mg_solver_set_rhs_host(s, u));
    } else OK(mg_solver_set_rhs_problem(s));
    OK(mg_solver_solve_gmres(s, restart));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "gmres", u, n);
    const int it = mg_solver_iterations(s);
    OK(mg_solver_solve_gmres(s, restart));                                  /* the same again */
    OK(mg_solver_get_solution(s, u2));
    if (mg_solver_iterations(s) != it || memcmp(u, u2, sizeof(double) * (size_t)n)) { fprintf(stderr, "the second solve_gmres differs\n"); return 5; }
    OK(mg_solver_solve_gmres(s, restart < 31 ? restart + 2 : 3));           /* another basis length: freed and allocated anew */
    REFUSED(mg_solver_solve_gmres(s, 0), "restart must be within");
    REFUSED(mg_solver_solve_gmres(s, MGK_KRYLOV_MAX), "restart must be within");
    s->cfg.nranks = 2;
    REFUSED(mg_solver_solve_gmres(s, restart), "one GPU");
    s->cfg.nranks = 1;
    s->cfg.precision = MG_PREC_MIXED;
    REFUSED(mg_solver_solve_gmres(s, restart), "not mixed precision");
    s->cfg.precision = MG_PREC_FP64;
    s->cfg.ksp_type = MG_KSP_CHEBYSHEV;
    REFUSED(mg_solver_solve_gmres(s, restart), "not Chebyshev");
    s->cfg.ksp_type = MG_KSP_RICHARDSON;
    OK(mg_solver_reset(s));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "after", u, n);
    fclose(f);
    free(u); free(u2);
    mg_solver_destroy(s);
    return 0;
}
