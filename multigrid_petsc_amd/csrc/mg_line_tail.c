/*
 * mg_line_tail.c -- the LDS-resident coarse levels of a line cycle in one launch (mg_config.line_tail = 1, include/mgsolve.h; DESIGN.md
 * section 8j).  The levels ltail .. L-1 of a solver with a line smoother (pc_type MG_PC_LINE_Y / _X / _ALT) run inside ONE kernel per cycle,
 * mgk_tail_cycle_line_f64: b of level ltail is there (the restriction from the level above wrote it), u of level ltail comes back after its
 * post-smoothing (src/solver.c:1536-1543 for those levels).  The kernel makes the plain sweeps of mg_line.c / mg_xline.c with the same bits,
 * so mg_solver.c picks ltail below every chunk period that applies (a chunked sweep rounds differently).  The level tables are the ones
 * mg_line_tables / mg_xline_tables uploaded at creation; nothing is allocated here.  b and u of level ltail never change for a line solver
 * (a line sweep swaps no buffers), so the launch may sit inside the recorded coarse-level graph.
 * This file is the only host code that names the kernel; mg_solver.c refers to it weakly (mg_solver_internal.h).
 */
#include "mg_solver_internal.h"
#include <stddef.h>

int mg_line_tail(mg_solver *s) {
    const int lt = s->ltail, nl = s->levels - lt, pc = s->cfg.pc_type;
    int n[8];
    const double *ct[8], *lt_[8], *gt[8], *qt[8], *xg[8];
    long xgs[8];
    if (lt < 1 || nl < 1 || nl > 8) return mgi_fail(MGK_EINVAL, "mg_line_tail: no tail levels");
    if (pc != MG_PC_LINE_Y && pc != MG_PC_LINE_X && pc != MG_PC_LINE_ALT) return mgi_fail(MGK_EINVAL, "mg_line_tail: not a line smoother");
    for (int q = 0; q < nl; q++) {
        const mg_level *L = &s->L[lt + q];
        n[q] = L->n;
        ct[q] = L->ctab; lt_[q] = L->ltab; gt[q] = L->gtab; qt[q] = L->qtab;
        xg[q] = L->xgtab; xgs[q] = L->xgs;
    }
    const int ysw = (pc != MG_PC_LINE_X), xsw = (pc != MG_PC_LINE_Y);
    mg_fset *F = &s->L[lt].f[0];
    CHK(mgk_tail_cycle_line_f64(s->ctx, &F->g, nl, n, pc, ct, ysw ? lt_ : NULL, ysw ? gt : NULL, ysw ? qt : NULL, xsw ? xg : NULL,
                                xsw ? xgs : NULL, s->cfg.scale, s->cfg.v[0], s->cfg.v[1], (const double *)F->b, (double *)F->u, NULL));
    return 0;
}
