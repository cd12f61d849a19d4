/* san_rbgs.c -- a red-black Gauss-Seidel solve through mg_solver.c + mg_rbgs.c over the host-memory stand-ins (tests/mock_mgk_rbgs.cpp), as a
 * plain executable so that it can be built with -fsanitize=address,undefined (tests/test_rbgs_cpu.py).  argv: npts levels mesh scale v0 v1
 * outfile.  Solves the manufactured problem, resets and solves again, asks for what the smoother is not built for on the live handle (fmg,
 * solve_fmg, solve_gmres: refused, and the handle still solves), then for what mg_solver_create refuses.  Writes the iterations, the residual
 * history and the solution of the solves as text (%.17g round-trips a double). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mgsolve.h"

#define OK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: rc=%d: %s\n", #call, rc_, mg_last_error()); return 2; } } while (0)

static void dump(FILE *f, mg_solver *s, const char *tag, const double *u, long n) {
    const int it = mg_solver_iterations(s);
    const double *rn = mg_solver_rnorm(s);
    fprintf(f, "%s_iters %d\n%s_rnorm", tag, it, tag);
    for (int q = 0; q <= it; q++) fprintf(f, " %.17g", rn[q]);
    fprintf(f, "\n%s_u", tag);
    for (long q = 0; q < n; q++) fprintf(f, " %.17g", u[q]);
    fprintf(f, "\n");
}

static int refused(mg_config c, const char *why) {
    mg_solver *s = NULL;
    const int rc = mg_solver_create(&s, &c, NULL);
    if (rc != MGK_EINVAL || s || !strstr(mg_last_error(), why)) {
        fprintf(stderr, "expected a refusal naming '%s', got rc=%d: %s\n", why, rc, mg_last_error());
        if (s) mg_solver_destroy(s);
        return 1;
    }
    return 0;
}

static int refused_call(int rc, const char *who) {
    if (rc != MGK_EINVAL || !strstr(mg_last_error(), who) || !strstr(mg_last_error(), "not the red-black Gauss-Seidel smoother")) {
        fprintf(stderr, "expected %s to refuse a red-black handle, got rc=%d: %s\n", who, rc, mg_last_error());
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 8) { fprintf(stderr, "usage: san_rbgs npts levels mesh scale v0 v1 outfile\n"); return 1; }
    mg_config c;
    mg_config_default(&c);
    c.dim = 2; c.npts = atoi(argv[1]); c.levels = atoi(argv[2]); c.mesh = atoi(argv[3]); c.scale = atof(argv[4]);
    c.v[0] = atoi(argv[5]); c.v[1] = atoi(argv[6]); c.maxiter = 100;
    c.pc_type = MG_PC_RBGS;
    mg_solver *s = NULL;
    OK(mg_solver_create(&s, &c, NULL));
    const long n = mg_solver_local_unknowns(s);
    double *u = (double *)malloc(sizeof(double) * (size_t)n);
    FILE *f = fopen(argv[7], "w");
    if (!u || !f) return 3;
    OK(mg_solver_set_rhs_problem(s));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "solve", u, n);
    OK(mg_solver_reset(s));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "again", u, n);
    /* refused on the live handle, each by its own message; the handle still solves */
    if (refused_call(mg_solver_fmg(s, 1), "mg_solver_fmg")) return 4;
    if (refused_call(mg_solver_solve_fmg(s, 1), "mg_solver_fmg")) return 4;
    if (refused_call(mg_solver_solve_gmres(s, 5), "mg_solver_solve_gmres")) return 4;
    OK(mg_solver_reset(s));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "after", u, n);
    fclose(f);
    free(u);
    mg_solver_destroy(s);
    /* refusals at creation: every one leaves nothing allocated (the leak check of the sanitizer run covers it) */
    mg_config r = c;
    r.dim = 3; r.npts = 17; r.levels = 3; r.mesh = 0;
    if (refused(r, "built for 2-D")) return 4;
    r = c; r.precision = MG_PREC_MIXED;
    if (refused(r, "not mixed precision")) return 4;
    r = c; r.ksp_type = MG_KSP_CHEBYSHEV; r.emin = 0.2; r.emax = 2.0;
    if (refused(r, "not Chebyshev")) return 4;
    r = c; r.nranks = 2;
    if (refused(r, "one GPU")) return 4;
    r = c; r.line_chunk = 4;
    if (refused(r, "must be 0 with pc_type rbgs")) return 4;
    r = c; r.xline_chunk = 16;
    if (refused(r, "must be 0 with pc_type rbgs")) return 4;
    r = c; r.line_tail = 1;
    if (refused(r, "must be 0 with pc_type rbgs")) return 4;
    r = c; r.pc_type = 5;
    if (refused(r, "pc_type must be")) return 4;
    return 0;
}
