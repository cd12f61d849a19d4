/* san_fmg.c -- full-multigrid sessions through mg_solver.c + mg_fmg.c over the host-memory stand-ins (tests/mock_mgk_fmg.cpp), as a plain
 * executable so that it can be built with -fsanitize=address,undefined (tests/test_random_sessions_cpu.py).
 * argv: dim npts levels v0 v1 scale fuse pair_min_n outfile.  One solver, the manufactured right-hand side, and on the same live handle:
 *   fmg(1) + cycles(3) | fmg(2) (no reset in between: FMG never reads the old iterate) | fmg(2) + cycles(3) | fmg(2) + cycles(1) | fmg(1) |
 *   fmg(1) + cycles(2) | solve, then fmg(2) + cycles(3) | solve_fmg(1) | reset + solve | the refusals (through the private header: fmg_check
 *   reads the configuration alone) | fmg(1) again, which must repeat the first one bit for bit.
 * Writes the histories and fields as text (%.17g round-trips a double); the test compares them with tests/fmg_reference.py and the oracle. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mg_solver_internal.h"

#define OK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: rc=%d: %s\n", #call, rc_, mg_last_error()); return 2; } } while (0)
#define REFUSED(call, msg) do { int rc_ = (call); if (rc_ != MGK_EINVAL || !strstr(mg_last_error(), msg)) { \
    fprintf(stderr, "%s: rc=%d: %s (expected a refusal with '%s')\n", #call, rc_, mg_last_error(), msg); return 4; } } while (0)

static int dump(FILE *f, mg_solver *s, const char *tag, double *u, long n) {
    if (mg_solver_sync(s) || mg_solver_get_solution(s, u)) { fprintf(stderr, "%s: %s\n", tag, mg_last_error()); return 2; }
    const int it = mg_solver_iterations(s);
    const double *rn = mg_solver_rnorm(s);
    fprintf(f, "%s_iters %d\n%s_bnorm %.17g\n%s_rnorm", tag, it, tag, mg_solver_bnorm(s), tag);
    for (int q = 0; q <= it; q++) fprintf(f, " %.17g", rn[q]);
    fprintf(f, "\n%s_u", tag);
    for (long q = 0; q < n; q++) fprintf(f, " %.17g", u[q]);
    fprintf(f, "\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 10) { fprintf(stderr, "usage: san_fmg dim npts levels v0 v1 scale fuse pair_min_n outfile\n"); return 1; }
    mg_config c;
    mg_config_default(&c);
    c.dim = atoi(argv[1]); c.npts = atoi(argv[2]); c.levels = atoi(argv[3]); c.v[0] = atoi(argv[4]); c.v[1] = atoi(argv[5]); c.scale = atof(argv[6]);
    c.fuse = atoi(argv[7]); c.pair_min_n = atoi(argv[8]);
    c.maxiter = 40;
    mg_solver *s = NULL;
    OK(mg_solver_create(&s, &c, NULL));
    const long n = mg_solver_local_unknowns(s);
    double *u = (double *)malloc(sizeof(double) * (size_t)n), *u1 = (double *)malloc(sizeof(double) * (size_t)n);
    FILE *f = fopen(argv[9], "w");
    if (!u || !u1 || !f) return 3;
    OK(mg_solver_set_rhs_problem(s));
    /* the sessions with which the random draw noticed the swap back to the recorded buffer roles missing (mg_fmg.c): the first level-0 cycle
     * records the coarse-level graph, a later FMG's stages swap u / tmp of a level inside it, and the cycles after that replay the recording */
    OK(mg_solver_fmg(s, 1));
    OK(mg_solver_cycles(s, 3));
    OK(dump(f, s, "fmg1c3", u, n));
    OK(mg_solver_fmg(s, 2));
    OK(dump(f, s, "fmg2", u, n));
    OK(mg_solver_fmg(s, 2));
    OK(mg_solver_cycles(s, 3));
    OK(dump(f, s, "fmg2c3", u, n));
    OK(mg_solver_fmg(s, 2));
    OK(mg_solver_cycles(s, 1));
    OK(dump(f, s, "fmg2c1", u, n));
    OK(mg_solver_fmg(s, 1));
    OK(dump(f, s, "fmg1", u1, n));
    OK(mg_solver_fmg(s, 1));
    OK(mg_solver_cycles(s, 2));
    OK(dump(f, s, "fmg1c2", u, n));
    OK(mg_solver_solve(s));
    OK(dump(f, s, "solve", u, n));
    OK(mg_solver_fmg(s, 2));
    OK(mg_solver_cycles(s, 3));
    OK(dump(f, s, "solve_fmg2c3", u, n));
    OK(mg_solver_solve_fmg(s, 1));
    OK(dump(f, s, "sfmg1", u, n));
    OK(mg_solver_reset(s));
    OK(mg_solver_solve(s));
    OK(dump(f, s, "after", u, n));
    REFUSED(mg_solver_fmg(NULL, 1), "null solver");
    REFUSED(mg_solver_fmg(s, 0), "nu must be >= 1");
    REFUSED(mg_solver_solve_fmg(s, -1), "nu must be >= 1");
    s->cfg.nranks = 2;
    REFUSED(mg_solver_fmg(s, 1), "one GPU");
    s->cfg.nranks = 1;
    s->cfg.precision = MG_PREC_MIXED;
    REFUSED(mg_solver_solve_fmg(s, 1), "not mixed precision");
    s->cfg.precision = MG_PREC_FP64;
    s->cfg.ksp_type = MG_KSP_CHEBYSHEV;
    REFUSED(mg_solver_fmg(s, 1), "not Chebyshev");
    s->cfg.ksp_type = MG_KSP_RICHARDSON;
    s->cfg.pc_type = MG_PC_LINE_Y;
    REFUSED(mg_solver_fmg(s, 1), "not the y-line smoother");
    s->cfg.pc_type = MG_PC_LINE_ALT;
    REFUSED(mg_solver_solve_fmg(s, 1), "not the x-line or alternating line smoothers");
    s->cfg.pc_type = MG_PC_JACOBI;
    s->cfg.mesh = 1;
    REFUSED(mg_solver_fmg(s, 1), "uniform mesh");
    s->cfg.mesh = 0;
    const int levels = s->levels;
    s->levels = 1;
    REFUSED(mg_solver_fmg(s, 1), "two levels or more");
    s->levels = levels;
    OK(mg_solver_fmg(s, 1));                                                /* the handle is as usable as before */
    OK(dump(f, s, "again", u, n));
    if (memcmp(u, u1, sizeof(double) * (size_t)n)) { fprintf(stderr, "fmg(1) after the refusals differs from the first fmg(1)\n"); return 5; }
    fclose(f);
    free(u); free(u1);
    mg_solver_destroy(s);
    return 0;
}
