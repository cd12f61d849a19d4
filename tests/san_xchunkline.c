/* san_xchunkline.c -- a line solve with the x sweeps in chunks through mg_solver.c + mg_line.c + mg_xline.c + mg_line_chunk.c + mg_xline_chunk.c
 * over the host-memory stand-ins (tests/mock_mgk_xchunkline.cpp), as a plain executable so that it can be built with
 * -fsanitize=address,undefined (tests/test_xchunkline_cpu.py).  argv: pc npts levels mesh scale xc yc rhsfile outfile (pc: 2 xline, 3 altline;
 * "-" as rhsfile: the manufactured right-hand side; otherwise (npts-2)^2 raw doubles).  First tries what xline_chunk is not built for
 * (every refused creation leaves nothing allocated: the leak check covers it), then solves, resets and solves again, and destroys.  Writes
 * the iterations, the residual history and the solution of both solves as text (%.17g round-trips a double). */
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

int main(int argc, char **argv) {
    if (argc != 10) { fprintf(stderr, "usage: san_xchunkline pc npts levels mesh scale xc yc rhsfile outfile\n"); return 1; }
    mg_config c;
    mg_config_default(&c);
    if (c.xline_chunk != 0 || c.line_chunk != 0) { fprintf(stderr, "mg_config_default: xline_chunk = %d\n", c.xline_chunk); return 4; }
    c.dim = 2; c.pc_type = atoi(argv[1]); c.npts = atoi(argv[2]); c.levels = atoi(argv[3]); c.mesh = atoi(argv[4]); c.scale = atof(argv[5]);
    c.xline_chunk = atoi(argv[6]); c.line_chunk = atoi(argv[7]);
    c.v[0] = 3; c.v[1] = 3; c.maxiter = 100;
    mg_config r = c;
    r.xline_chunk = -16;
    if (refused(r, "xline_chunk must be")) return 4;
    r = c; r.xline_chunk = 8;
    if (refused(r, "xline_chunk must be")) return 4;
    r = c; r.xline_chunk = 40;
    if (refused(r, "xline_chunk must be")) return 4;
    r = c; r.line_chunk = 0; r.pc_type = MG_PC_JACOBI;
    if (refused(r, "not jacobi or yline")) return 4;
    r = c; r.pc_type = MG_PC_LINE_Y;
    if (refused(r, "not jacobi or yline")) return 4;
    r = c; r.dim = 3; r.npts = 17; r.levels = 3; r.mesh = 0;
    if (refused(r, "built for 2-D")) return 4;
    r = c; r.precision = MG_PREC_MIXED;
    if (refused(r, "not mixed precision")) return 4;
    r = c; r.ksp_type = MG_KSP_CHEBYSHEV; r.emin = 0.2; r.emax = 2.0;
    if (refused(r, "not Chebyshev")) return 4;
    r = c; r.nranks = 2;
    if (refused(r, "one GPU")) return 4;
    mg_solver *s = NULL;
    OK(mg_solver_create(&s, &c, NULL));
    const long n = mg_solver_local_unknowns(s);
    double *u = (double *)malloc(sizeof(double) * (size_t)n);
    FILE *f = fopen(argv[9], "w");
    if (!u || !f) return 3;
    if (strcmp(argv[8], "-")) {
        FILE *fb = fopen(argv[8], "rb");
        if (!fb || fread(u, sizeof(double), (size_t)n, fb) != (size_t)n) return 3;
        fclose(fb);
        OK(mg_solver_set_rhs_host(s, u));
    } else OK(mg_solver_set_rhs_problem(s));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "solve", u, n);
    OK(mg_solver_reset(s));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "again", u, n);
    fclose(f);
    free(u);
    mg_solver_destroy(s);
    return 0;
}
