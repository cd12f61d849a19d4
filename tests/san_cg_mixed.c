/* san_cg_mixed.c -- CG solves over the fp32 cycle through mg_solver.c + mg_cg.c + mg_cg_mixed.c over the host-memory stand-ins
 * (tests/mock_mgk_cg_mixed.cpp), as a plain executable so that it can be built with -fsanitize=address,undefined (tests/test_cg_mixed_cpu.py).
 * argv: dim npts levels scale v0 v1 maxiter rhsfile outfile (rhsfile: raw doubles of the compact right-hand side, "-" = the manufactured
 * one); the solver is created with precision = MG_PREC_MIXED.  Runs solve_cg_mixed, again, then once with an allocation that fails (nothing may stay allocated: leak detection is on), checks the
 * refusals (through the private header: the check reads the configuration alone) with a working handle after each, then reset + solve; writes
 * the histories and fields as text (%.17g round-trips a double). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mg_solver_internal.h"

extern void mock_cg_fail_malloc(long nth);

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
    if (argc != 10) { fprintf(stderr, "usage: san_cg_mixed dim npts levels scale v0 v1 maxiter rhsfile outfile\n"); return 1; }
    mg_config c;
    mg_config_default(&c);
    c.dim = atoi(argv[1]); c.npts = atoi(argv[2]); c.levels = atoi(argv[3]); c.scale = atof(argv[4]);
    c.v[0] = atoi(argv[5]); c.v[1] = atoi(argv[6]);
    c.maxiter = atoi(argv[7]);
    c.precision = MG_PREC_MIXED;
    mg_solver *s = NULL;
    OK(mg_solver_create(&s, &c, NULL));
    const long n = mg_solver_local_unknowns(s);
    double *u = (double *)malloc(sizeof(double) * (size_t)n), *u2 = (double *)malloc(sizeof(double) * (size_t)n);
    FILE *f = fopen(argv[9], "w");
    if (!u || !u2 || !f) return 3;
    /* the third of the five fields does not fit: refused, nothing stays allocated, and the next call allocates anew */
    OK(mg_solver_set_rhs_problem(s));
    mock_cg_fail_malloc(3);
    REFUSED(mg_solver_solve_cg_mixed(s), "needs 5 fine-level fields of");
    if (strcmp(argv[8], "-")) {
        FILE *r = fopen(argv[8], "rb");
        if (!r || fread(u, sizeof(double), (size_t)n, r) != (size_t)n) return 3;
        fclose(r);
        OK(mg_solver_set_rhs_host(s, u));
    }
    OK(mg_solver_solve_cg_mixed(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "cg", u, n);
    fprintf(f, "cg_breakdown %d\n", mg_solver_cg_breakdown(s));
    const int it = mg_solver_iterations(s);
    OK(mg_solver_solve_cg_mixed(s));                                              /* the same again */
    OK(mg_solver_get_solution(s, u2));
    if (mg_solver_iterations(s) != it || memcmp(u, u2, sizeof(double) * (size_t)n)) { fprintf(stderr, "the second solve_cg_mixed differs\n"); return 5; }
    REFUSED(mg_solver_solve_cg_mixed(NULL), "null solver");
    s->cfg.nranks = 2;
    REFUSED(mg_solver_solve_cg_mixed(s), "one GPU");
    s->cfg.nranks = 1;
    s->cfg.precision = MG_PREC_FP64;
    REFUSED(mg_solver_solve_cg_mixed(s), "built for a mixed-precision solver");
    s->cfg.precision = MG_PREC_MIXED;
    REFUSED(mg_solver_solve_cg(s), "not mixed precision");                  /* the fp64 entry point still refuses a mixed solver */
    s->cfg.ksp_type = MG_KSP_CHEBYSHEV;
    REFUSED(mg_solver_solve_cg_mixed(s), "not Chebyshev");
    s->cfg.ksp_type = MG_KSP_RICHARDSON;
    s->cfg.pc_type = MG_PC_LINE_Y;
    REFUSED(mg_solver_solve_cg_mixed(s), "built for point Jacobi");
    s->cfg.pc_type = MG_PC_RBGS;
    REFUSED(mg_solver_solve_cg_mixed(s), "built for point Jacobi");
    s->cfg.pc_type = MG_PC_JACOBI;
    s->cfg.mesh = 1;
    REFUSED(mg_solver_solve_cg_mixed(s), "uniform mesh");
    s->cfg.mesh = 0;
    OK(mg_solver_solve_cg_mixed(s));                                              /* the handle is as usable as before */
    OK(mg_solver_get_solution(s, u2));
    if (mg_solver_iterations(s) != it || memcmp(u, u2, sizeof(double) * (size_t)n)) { fprintf(stderr, "solve_cg_mixed after the refusals differs\n"); return 5; }
    OK(mg_solver_reset(s));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "after", u, n);
    fclose(f);
    free(u); free(u2);
    mg_solver_destroy(s);
    return 0;
}
