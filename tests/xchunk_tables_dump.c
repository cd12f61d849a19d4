/* xchunk_tables_dump.c -- the host tables of the x-line sweep in chunks (csrc/mg_xline_chunk.c), written out: mg_solver.c + mg_comm.c + mg_line.c +
 * mg_xline.c + mg_line_chunk.c + mg_xline_chunk.c over the host-memory stand-ins of the kernel ABI (tests/mock_mgk_xchunkline.cpp), as a plain
 * executable (tests/test_xchunkline_cpu.py).  argv: npts levels mesh c outfile.  Creates a 2-D solver with pc_type xline and xline_chunk = c and
 * writes, one record per line and every double as %a (exact):
 *   ctab L N v.. (N rows x 5) | chunk L N K rows gstride sstride | g L v.. | v | w (rows x N each, row by row, the padding left out) |
 *   pad L v.. (the padding of g, v and w: all of it) | SL | SG | SQ L v.. (rows x K each, row by row)                  a level with n >= c
 *   ctab L N v..              | plain L N                                                                               a level with n < c
 * rows = 1 and the strides 0 on the uniform mesh.  Under the stand-ins the solver's device pointers are host memory, so the tables are read
 * in place.  The test compares them with tests/xchunkline_reference.tables on the same row table. */
#include <stdio.h>
#include <stdlib.h>
#include "mg_solver_internal.h"

#define OK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: rc=%d: %s\n", #call, rc_, mg_last_error()); return 2; } } while (0)

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: xchunk_tables_dump npts levels mesh c outfile\n"); return 1; }
    mg_config c;
    mg_config_default(&c);
    c.dim = 2; c.npts = atoi(argv[1]); c.levels = atoi(argv[2]); c.mesh = atoi(argv[3]); c.xline_chunk = atoi(argv[4]);
    c.v[0] = 3; c.v[1] = 3; c.maxiter = 10;
    c.pc_type = MG_PC_LINE_X;
    mg_solver *s = NULL;
    OK(mg_solver_create(&s, &c, NULL));
    FILE *f = fopen(argv[5], "w");
    if (!f) return 3;
    for (int l = 0; l < s->levels; l++) {
        const mg_level *L = &s->L[l];
        const long n = L->n, K = n / c.xline_chunk, rows = c.mesh ? n : 1, n16 = (n + 15) / 16 * 16;
        const long gs = c.mesh ? n16 : 0, ss = c.mesh ? n16 : 0, T = rows * n16, KS = c.mesh ? K * ss : K;
        fprintf(f, "ctab %d %ld", l, n);
        for (long q = 0; q < 5 * n; q++) fprintf(f, " %a", L->ctab[q]);
        fprintf(f, "\n");
        if (!L->xchunktab) { fprintf(f, "plain %d %ld\n", l, n); continue; }
        if (!L->xchunksep || gs != mg_xline_stride((int)n, !c.mesh)) return 4;
        fprintf(f, "chunk %d %ld %ld %ld %ld %ld\n", l, n, K, rows, gs, ss);
        const char *tags[3] = {"g", "v", "w"}, *stags[3] = {"SL", "SG", "SQ"};
        for (int t = 0; t < 3; t++) {
            fprintf(f, "%s %d", tags[t], l);
            for (long i = 0; i < rows; i++) for (long j = 0; j < n; j++) fprintf(f, " %a", L->xchunktab[t * T + i * gs + j]);
            fprintf(f, "\n");
        }
        fprintf(f, "pad %d", l);
        for (int t = 0; t < 3; t++) for (long i = 0; i < rows; i++) for (long j = n; j < n16; j++) fprintf(f, " %a", L->xchunktab[t * T + i * n16 + j]);
        fprintf(f, "\n");
        for (int t = 0; t < 3; t++) {
            fprintf(f, "%s %d", stags[t], l);
            for (long i = 0; i < rows; i++) for (long q = 0; q < K; q++) fprintf(f, " %a", L->xchunktab[3 * T + t * KS + (ss ? q * ss + i : q)]);
            fprintf(f, "\n");
        }
    }
    fclose(f);
    mg_solver_destroy(s);
    return 0;
}
