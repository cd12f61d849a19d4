/* ref_tables_dump.c -- the host arithmetic of the product's own driver, written out: mg_solver.c + mg_comm.c + mg_line.c over the host-memory
 * stand-ins of the kernel ABI (tests/mock_mgk_line.cpp), as a plain executable so that it can also be built with -fsanitize=address,undefined
 * (tests/test_reference_fixtures_cpu.py).  argv: npts levels mesh outfile.  Creates a 2-D solver, calls mg_solver_set_rhs_problem and writes,
 * one record per line and every double as %a (exact):
 *   coef L c0..c4 | dinv L v | h L v | ctab L N v.. (N rows x 5, stretched meshes only) | dtab L N v.. | b N v.. (level 0, N x N, row-major)
 * Under the stand-ins the solver's device pointers are host memory, so the tables are read in place.  The test compares them with what the
 * reference handed to MatSetValue / VecSetValue (tests/golden/ref_assembly.npz). */
#include <stdio.h>
#include <stdlib.h>
#include "mg_solver_internal.h"

#define OK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: rc=%d: %s\n", #call, rc_, mg_last_error()); return 2; } } while (0)

static void row(FILE *f, const char *tag, int l, long n, const double *v, long count) {
    fprintf(f, "%s %d", tag, l);
    if (n >= 0) fprintf(f, " %ld", n);
    for (long q = 0; q < count; q++) fprintf(f, " %a", v[q]);
    fprintf(f, "\n");
}

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: ref_tables_dump npts levels mesh outfile\n"); return 1; }
    mg_config c;
    mg_config_default(&c);
    c.dim = 2; c.npts = atoi(argv[1]); c.levels = atoi(argv[2]); c.mesh = atoi(argv[3]);
    c.v[0] = 3; c.v[1] = 3; c.maxiter = 10;
    mg_solver *s = NULL;
    OK(mg_solver_create(&s, &c, NULL));
    OK(mg_solver_set_rhs_problem(s));
    FILE *f = fopen(argv[4], "w");
    if (!f) return 3;
    for (int l = 0; l < s->levels; l++) {
        const mg_level *L = &s->L[l];
        row(f, "coef", l, -1, L->coef, 5);
        row(f, "dinv", l, -1, &L->dinv, 1);
        row(f, "h", l, -1, &L->h, 1);
        if (L->ctab) row(f, "ctab", l, L->n, L->ctab, 5 * (long)L->n);
        if (L->dtab) row(f, "dtab", l, L->n, L->dtab, L->n);
    }
    const mg_fset *F = &s->L[0].f[0];
    const double *b = (const double *)F->b;
    fprintf(f, "b %d", F->g.ny);
    for (int i = 0; i < F->g.ny; i++)
        for (int j = 0; j < F->g.nx; j++) fprintf(f, " %a", b[F->g.org + (long)i * F->g.pitch + j]);
    fprintf(f, "\n");
    fclose(f);
    mg_solver_destroy(s);
    return 0;
}
