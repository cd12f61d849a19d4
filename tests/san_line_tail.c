/* san_line_tail.c -- a line solve with mg_config.line_tail = 1 through mg_solver.c + mg_line.c + mg_xline.c + mg_line_tail.c over the
 * host-memory stand-ins (tests/mock_mgk_line_tail.cpp), as a plain executable so that it can be built with -fsanitize=address,undefined
 * (tests/test_line_tail_cpu.py).  argv: pc_type (1: y-line, 2: x-line, 3: alternating) npts levels mesh scale rhsfile outfile ("-" as
 * rhsfile: the manufactured right-hand side; otherwise (npts-2)^2 raw doubles).  Solves with the tail, resets and solves again, solves
 * with line_tail = 0, then tries what line_tail is not built for.  Writes the tail level, the iterations, the residual history and the
 * solution of the three solves as text (%.17g round-trips a double). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mgsolve.h"

#define OK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: rc=%d: %s\n", #call, rc_, mg_last_error()); return 2; } } while (0)

static void dump(FILE *f, mg_solver *s, const char *tag, const double *u, long n) {
    const int it = mg_solver_iterations(s);
    const double *rn = mg_solver_rnorm(s);
    fprintf(f, "%s_tail_level %d\n%s_iters %d\n%s_rnorm", tag, mg_solver_tail_level(s), tag, it, tag);
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

static int rhs(mg_solver *s, const char *file, double *buf, long n) {
    if (!strcmp(file, "-")) return mg_solver_set_rhs_problem(s);
    FILE *fb = fopen(file, "rb");
    if (!fb || fread(buf, sizeof(double), (size_t)n, fb) != (size_t)n) return 3;
    fclose(fb);
    return mg_solver_set_rhs_host(s, buf);
}

int main(int argc, char **argv) {
    if (argc != 8) { fprintf(stderr, "usage: san_line_tail pc_type npts levels mesh scale rhsfile outfile\n"); return 1; }
    argv++;
    mg_config c;
    mg_config_default(&c);
    if (c.line_tail != 0) { fprintf(stderr, "line_tail is not off by default\n"); return 5; }
    c.dim = 2; c.npts = atoi(argv[1]); c.levels = atoi(argv[2]); c.mesh = atoi(argv[3]); c.scale = atof(argv[4]);
    c.v[0] = 3; c.v[1] = 3; c.maxiter = 100;
    c.pc_type = atoi(argv[0]);
    c.line_tail = 1;
    mg_solver *s = NULL;
    OK(mg_solver_create(&s, &c, NULL));
    const long n = mg_solver_local_unknowns(s);
    double *u = (double *)malloc(sizeof(double) * (size_t)n);
    FILE *f = fopen(argv[6], "w");
    if (!u || !f) return 3;
    OK(rhs(s, argv[5], u, n));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "solve", u, n);
    OK(mg_solver_reset(s));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "again", u, n);
    mg_solver_destroy(s);
    s = NULL;
    mg_config p = c;
    p.line_tail = 0;
    OK(mg_solver_create(&s, &p, NULL));
    OK(rhs(s, argv[5], u, n));
    OK(mg_solver_solve(s));
    OK(mg_solver_get_solution(s, u));
    dump(f, s, "plain", u, n);
    mg_solver_destroy(s);
    fclose(f);
    free(u);
    /* refusals: every one leaves nothing allocated (the leak check of the sanitizer run covers it) */
    mg_config r = c;
    r.line_tail = 2;
    if (refused(r, "line_tail must be 0 (off) or 1")) return 4;
    r = c; r.line_tail = -1;
    if (refused(r, "line_tail must be 0 (off) or 1")) return 4;
    r = c; r.pc_type = MG_PC_JACOBI;
    if (refused(r, "line_tail goes with the line smoothers")) return 4;
    r = c; r.dim = 3; r.npts = 17; r.levels = 3; r.mesh = 0;
    if (refused(r, "built for 2-D")) return 4;
    /* accepted, and the tail stays off: one level would be left */
    r = c; r.levels = 2;
    s = NULL;
    OK(mg_solver_create(&s, &r, NULL));
    if (mg_solver_tail_level(s) != 0) { fprintf(stderr, "a tail of one level\n"); return 4; }
    mg_solver_destroy(s);
    return 0;
}
