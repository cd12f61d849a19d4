/*
 * mg_solver_internal.h -- the solver's state and the cycle steps that the full-multigrid driver (mg_fmg.c), the GMRES driver (mg_gmres.c)
 * and the CG driver (mg_cg.c) build on.  Private to libmgpetsc.so: not installed, not part of the C API (include/mgsolve.h).  Everything declared here is DEFINED in
 * mg_solver.c, which references no symbol of mg_fmg.c, mg_gmres.c or mg_cg.c (the host tests link mg_solver.c without them, against a mock of the
 * kernel ABI).
 */
#ifndef MG_SOLVER_INTERNAL_H
#define MG_SOLVER_INTERNAL_H
#include "mgsolve.h"
#include "mg_comm.h"
#include "mg_cheby_coefs.h"

#define MG_MAX_LEVELS 32
#define MG_MAX_TIMERS 4096
#define MG_CG_FIELDS 5

/* fuse bits mg_solver_create clears (include/mgsolve.h: mg_fuse_bits) */
/* y-line Jacobi: every pass that bakes POINT Jacobi into its kernel (bits 1, 3, 5, 8-15); the fused residual + norm and residual + restriction stay */
#define MG_FUSE_POINT_JACOBI_PASSES (MG_FUSE_PROLONG_SWEEP | MG_FUSE_NORM_SWEEP | MG_FUSE_PAIRS | MG_FUSE_COARSE_ZERO_SWEEP | MG_FUSE_LDS_TAIL | \
                                     MG_FUSE_SWEEP_RESTRICT | MG_FUSE_ZERO_TRIPLE | MG_FUSE_PROLONG_PAIR | MG_FUSE_TRIPLE_2D | \
                                     MG_FUSE_PROLONG_PAIR_SLAB | MG_FUSE_CHEBY | MG_FUSE_TRIPLE_MID | MG_FUSE_TRIPLE_NORM)
/* row-dependent coefficients (-mesh 1/2; 2-D, fp64): the two passes that exist in 3-D alone and have no row-table form */
#define MG_FUSE_NO_ROW_TABLE_FORM   (MG_FUSE_MIXED_CORRECT | MG_FUSE_RES_RESTRICT_SMALL)

/* the fields of one level in one precision (index 0: fp64, 1: fp32) */
typedef struct mg_fset {
    mgk_geom g;             /* local geometry in elements of that precision */
    void *u, *b, *rv, *tmp;
    int guess_nonzero;      /* KSPSetInitialGuessNonzero state of ksp[l] (src/solver.c:1532,1537,1543) */
    int u_ghost_ok;         /* z ghost planes of `u` hold the neighbours' current boundary planes */
    int u_ghost_pending;    /* ... but the exchange is still in flight on the comm stream */
    int jz_ready;           /* tmp already holds the first sweep from a zero guess (written by the fused residual+restriction) */
    int last_sweep_pending; /* pre-smoothing stopped one sweep short: the restriction that follows makes it (mgk_sweep_residual_restrict_f64) */
    int b_ghost_ok;         /* z ghost planes of `b` hold the neighbours' boundary planes (two-sweep passes on slabs) */
    int pre_done;           /* FMG (mg_fmg.c): u already holds the first pre_done sweeps of the next smoothing from a non-zero guess (made by the
                             * interpolation kernel); smooth() starts after them */
    void *far;              /* distributed levels: field of geometry gfar = (nx, ny, 2) for the neighbours' SECOND planes of u */
    void *far2, *bfar;      /* fp64, fuse bit 10: same geometry; hi ghost = the rank above's THIRD plane of u / SECOND plane of b (sweep fused
                             * with residual + restriction on a slab: mgk_sweep_residual_restrict_slab_f64) */
    int bfar_ok;            /* bfar's hi ghost plane is valid (b of a level changes only when the restriction above rewrites it) */
    mgk_geom gfar;
} mg_fset;

/* u of this field set was just rewritten: its ghost planes are stale and no exchange of them is travelling */
static inline void mgi_u_rewritten(mg_fset *F) { F->u_ghost_ok = 0; F->u_ghost_pending = 0; }

typedef struct mg_level {
    int n;                  /* unknowns per side of the whole grid */
    int z0, nzl;            /* owned planes [z0, z0+nzl) (3-D); whole grid when replicated / 2-D */
    int nz_min;             /* fewest planes any rank owns on this level: every choice between code paths that differ in their
                             * exchanges is made on it, never on the own slab size, so that all ranks take the same path */
    int distributed;
    double coef[7], dinv, h;
    double *ctab, *dtab;    /* -mesh 1/2 (2-D): device tables, 5 coefficients {(i-1), W, C, E, (i+1)} and 1/diag per grid row */
    mg_fset f[2];
    double *p2;             /* Chebyshev: third recurrence vector (fp64) */
    double *ltab, *gtab, *qtab;   /* y-line Jacobi (pc_type MG_PC_LINE_Y): device tables of the factorised y-tridiagonal part, n doubles each
                                   * (multipliers, 1 / pivot, N / pivot); ctab / dtab then exist on the uniform mesh too */
    double *xgtab; long xgs;      /* x-line Jacobi (MG_PC_LINE_X / MG_PC_LINE_ALT): device table 1 / pivot of the factorised x-tridiagonal part,
                                   * rows at a stride of xgs doubles (0: one row for every grid row -- the uniform mesh) */
    double *chunktab;             /* y-line sweeps in chunks (mg_config.line_chunk = c, mg_line_chunk.c): one device array [l g q v w | L G Q], five
                                   * tables of n doubles and three of n / c; NULL on a level with n < c, which keeps the plain sweep */
    double *xchunktab, *xchunksep; /* x-line sweeps in chunks (mg_config.xline_chunk = c, mg_xline_chunk.c): one device array [g | v | w | SL SG SQ]
                                   * and the separator workspace of 4 (n / c) rows; NULL on a level with n < c, which keeps the plain sweep */
} mg_level;

struct mg_solver {
    mg_config cfg;
    mgk_ctx *ctx;
    mg_comm *comm;
    int levels, ldist;      /* ldist: number of distributed (finest) levels; 0 when nranks == 1 */
    mg_level L[MG_MAX_LEVELS];
    int *zstart;            /* plane starts of the first replicated level's producers (nranks+1) */
    double *rnorm;          /* maxiter+1 */
    int rnorm_cap;
    int iter;
    double bnorm, rchk;
    int started;
    int deferring;          /* mg_solver_cycles: norms are deposited on the device and read once at the end */
    double *d_norms; int d_norms_cap;
    double *pin; int pin_cap; /* pinned host landing area of the reduced norms */
    int spec_valid;         /* > 0: level-0 tmp holds that many sweeps of u, made by the sweep(s)+norm kernel that closed the last cycle */
    int sweep_owed;         /* fuse bit 12: the post-smoothing of level 0 stopped one sweep short (prolongation + two sweeps in one pass); the
                             * pass that evaluates the norm makes that sweep first */
    int last_cycle;         /* the caller knows (fixed cycle count) or expects (contraction so far) that this cycle is the last one: no sweep is
                             * owed and no speculative sweep is made -- the norm comes from the store-free residual + norm pass */
    int iterate_behind;     /* ... and after that pass u is still ONE sweep behind the iterate the norm belongs to (it was never stored:
                             * tmp holds the sweep after it); finalize_iterate() makes the sweep if the iteration stops here */
    double solve_seconds;
    int lgraph;             /* levels >= lgraph form the launch-bound coarse part replayed as one HIP graph (0: off) */
    int ltail;              /* levels >= ltail (n <= 15 in 3-D, <= 63 in 2-D) run as ONE kernel with their fields in LDS (0: off); line smoothers:
                             * mg_config.line_tail, below every chunk period that applies */
    void *coarse_graph[2];  /* one recording per precision */
    void *graph_u[2], *graph_tmp[2];   /* u / tmp of the level that feeds the recording, as the recorded kernels know them */
    int graph_rerecorded;   /* recordings thrown away because those pointers had changed (0 in every default configuration) */
    int prolong_triple_launches[MG_MAX_LEVELS];   /* launches of the prolongation + three-sweep pass per level since the solver was created (mg_triple.c) */
    int triple_norm_launches;   /* launches of the norm + three-sweep pass of level 0 (fuse bit 17) since the solver was created (mg_triple.c) */
    /* profiling */
    int prof_on, prof_n;
    void *timers[MG_MAX_TIMERS];
    unsigned char timer_kind[MG_MAX_TIMERS];
    int prof_kind;          /* kind of the next timer: 0 plain sweep, 1 two sweeps in one pass */
    int ntimers_created;
    /* GMRES (mg_gmres.c): fine-level fields allocated at the first mg_solver_solve_gmres for a restart length -- basis (restart + 1), x, w, the
     * caller's b -- and the device slots of the Hessenberg column; freed by mg_solver_destroy */
    void *gm_field[MGK_KRYLOV_MAX + 3];
    int gm_nfields, gm_restart;
    double *gm_hdev;
    /* conjugate gradients (mg_cg.c): x, p, the other p, q and the caller's b, the device slot of r . z and the reduction workspace of the two
     * fused passes, allocated at the first mg_solver_solve_cg; freed by mg_solver_destroy, the workspace through cg_ws_free (set by mg_cg.c,
     * the only file that knows what it is) */
    void *cg_field[MG_CG_FIELDS];
    double *cg_rho_dev;
    void *cg_ws;
    void (*cg_ws_free)(mgk_ctx *ctx, void *ws);
    int cg_breakdown;       /* the step (1-based) in which the last mg_solver_solve_cg broke down; 0: none */
};

/* KSPCHEBYSHEV on the fused cycle (fuse bit 15): mg_cheby.c holds the only calls of the mgk_cheby3_2d_* / mgk_tail_cycle_cheby_f64 kernels.
 * mg_solver.c reaches it through these WEAK references and tests them for NULL: a build without mg_cheby.c (the host tests link mg_solver.c
 * against a stand-in of the kernel ABI that knows none of those kernels) needs no new symbol and runs Chebyshev step by step as before */
enum { MG_CHEBY_ZERO = 0, MG_CHEBY_PLAIN = 1, MG_CHEBY_PROLONG = 2, MG_CHEBY_NORM = 3 };
/* KSPSolve(max_it = 3) on level l in one pass, u (from zero / as it is / + P u_{l+1}) -> tmp; NORM: and *sumsq = ||b - A u||^2 of the input.
 * The caller swaps u / tmp */
extern int mg_cheby_pass(mg_solver *s, int l, int kind, double *sumsq) __attribute__((weak));
extern int mg_cheby_tail(mg_solver *s) __attribute__((weak));      /* the levels ltail .. L-1 of one cycle in one kernel */

/* y-line Jacobi (pc_type MG_PC_LINE_Y): mg_line.c holds the only calls of mgk_line_forward_f64 / mgk_line_backward_f64, reached like mg_cheby.c
 * through WEAK references: a build without it (the host tests' links of mg_solver.c against the plain stand-in of the kernel ABI) needs no new
 * symbol, and mg_solver_create refuses the line smoother there */
extern int mg_line_tables(mg_solver *s, int l, const double *ctab_host) __attribute__((weak));   /* factorise and upload level l's tables */
extern int mg_line_smooth(mg_solver *s, int l, int maxit) __attribute__((weak));   /* KSPSolve on level l: maxit sweeps in place, no swap */
/* x-line Jacobi and alternating line relaxation (MG_PC_LINE_X / MG_PC_LINE_ALT): mg_xline.c holds the only calls of mgk_xline_forward_f64 /
 * mgk_xline_backward_f64 and makes the y sweeps of the alternation through mg_line_smooth; reached through WEAK references in the same way */
extern int mg_xline_tables(mg_solver *s, int l, const double *ctab_host) __attribute__((weak));  /* factorise and upload level l's x table */
extern int mg_xline_smooth(mg_solver *s, int l, int maxit) __attribute__((weak));  /* KSPSolve on level l: x sweeps, or y and x in turn */
/* the y sweeps in chunks (mg_config.line_chunk >= 2): mg_line_chunk.c holds the only calls of the four mgk_line_chunk_*_f64 kernels; mg_solver.c
 * (the tables) and mg_line.c (the sweeps of a level that has them) reach it through WEAK references, and mg_solver_create refuses line_chunk > 0
 * in a build without it */
extern int mg_line_chunk_tables(mg_solver *s, int l, const double *ctab_host) __attribute__((weak));   /* level l's tables; none when n < c */
extern int mg_line_chunk_smooth(mg_solver *s, int l, int maxit) __attribute__((weak));   /* mg_line_smooth on a level with chunk tables */
/* the x sweeps in chunks (mg_config.xline_chunk > 0): mg_xline_chunk.c holds the only calls of the four mgk_xline_chunk_*_f64 kernels; mg_solver.c
 * (the tables) and mg_xline.c (the x sweeps of a level that has them) reach it through WEAK references, and mg_solver_create refuses
 * xline_chunk > 0 in a build without it */
extern int mg_xline_chunk_tables(mg_solver *s, int l, const double *ctab_host) __attribute__((weak));  /* level l's tables; none when n < c */
extern int mg_xline_chunk_smooth(mg_solver *s, int l, int maxit) __attribute__((weak));  /* maxit x sweeps on a level with chunk tables */
/* the LDS-resident coarse levels of a line cycle in one launch (mg_config.line_tail = 1): mg_line_tail.c holds the only call of
 * mgk_tail_cycle_line_f64; mg_solver.c (tail()) reaches it through a WEAK reference, and mg_solver_create refuses line_tail = 1 in a build
 * without it */
extern int mg_line_tail(mg_solver *s) __attribute__((weak));      /* the levels ltail .. L-1 of one cycle in one kernel */
/* red-black Gauss-Seidel (pc_type MG_PC_RBGS): mg_rbgs.c holds the only calls of mgk_rbgs_2d_f64 / mgk_prolong_rbgs_2d_f64, reached through WEAK
 * references in the same way; mg_solver_create refuses the smoother in a build without it.  Every pass writes tmp and swaps u / tmp */
extern int mg_rbgs_smooth(mg_solver *s, int l, int maxit) __attribute__((weak));   /* KSPSolve on level l: ceil(maxit / 2) passes */
extern int mg_rbgs_prolong_smooth(mg_solver *s, int l, int maxit) __attribute__((weak));   /* u_l <- RB^maxit(u_l + P u_{l+1}), maxit >= 1: the first pass prolongs */
/* the middle pass of the 75-byte 3-D fine level (fuse bit 16, MG_FUSE_TRIPLE_MID): mg_triple.c holds the only calls of mgk_jacobi3_sumsq_mid_f64 /
 * mgk_jacobi3_mid_ok_f64 (include/mgk_sweep3.h), reached through WEAK references in the same way: a build without it runs the 91-byte passes */
extern int mg_triple_mid_fits(const mg_solver *s) __attribute__((weak));          /* level 0 has a shape the pass is built for */
extern int mg_triple_mid_pass(mg_solver *s, double *sumsq) __attribute__((weak)); /* level 0: tmp = J(J(J(u))), *sumsq = ||b - A J(u)||^2 */
/* the same bit, the generic post-smoothing of a 511- / 1023-wide level outside the coarse-level graph: the prolongation, its correction and three
 * sweeps in one pass (mgk_prolong_jacobi3_f64, named by mg_triple.c alone) instead of prolongation + sweep and a two-sweep pass */
extern int mg_triple_prolong_fits(const mg_solver *s, int l) __attribute__((weak));   /* levels l, l + 1 have shapes the pass is built for */
extern int mg_triple_prolong_pass(mg_solver *s, int l) __attribute__((weak));         /* level l: tmp = J(J(J(u + P u_{l+1}))); counts the launch */
/* fuse bit 17 (MG_FUSE_TRIPLE_NORM): the norm of level 0's stored iterate and the three pre-smoothing sweeps of the next cycle in one stacked pass
 * (mgk_jacobi3_sumsq_f64 on a shape mg_triple_mid_fits accepts), reached through a WEAK reference like the other two passes of mg_triple.c */
extern int mg_triple_norm_pass(mg_solver *s, double *sumsq) __attribute__((weak));    /* level 0: tmp = J(J(J(u))), *sumsq = ||b - A u||^2; counts the launch */
long mg_xline_stride(int n, int uniform);                                         /* row stride of the x table (mg_xline.c) */
void mg_xline_factor(int n, int rows, const double *ctab, long gs, double *g);     /* the x table on the host (mg_xline.c) */

/* the steps of mg_solver.c, for mg_fmg.c (fp64, one rank) */
int    mgi_fail(int code, const char *what);            /* records the message for mg_last_error(), returns code */
/* a failed call of the kernel layer ends the calling function with its code, the call's text recorded as the message */
#define CHK(call) do { int rc_ = (call); if (rc_) return mgi_fail(rc_, #call); } while (0)
int    mgi_upload(mg_solver *s, const double *h, size_t n, double **d);   /* a new device array holding n host doubles */
double mgi_wall(void);
int    mgi_start(mg_solver *s);                          /* src/solver.c:1512-1523: ||b||, u0 = 0, rnorm[0], every level flag reset, iter = 0 */
int    mgi_smooth(mg_solver *s, int l, int maxit);       /* KSPSolve on level l (guess as L[l].f[0].guess_nonzero says), no restriction follows */
int    mgi_vcycle_rooted(mg_solver *s, int l);           /* one V-cycle on the levels l .. L-1 (l >= 1) from the guess in u_l, without the graph */
int    mgi_vcycle_once(mg_solver *s);                    /* one iteration of the solve loop (cycle rooted at level 0 + the norm), iter += 1 */
int    mgi_iterate(mg_solver *s);                        /* the solve loop under the stop rule of src/solver.c:1530, from the current state */
int    mgi_finalize(mg_solver *s);                       /* materialise the iterate the last norm belongs to */
/* the V-cycle as a linear operator (mg_gmres.c, mg_cg.c): ONE cycle rooted at level 0 from the zero guess on whatever level 0's b holds, no norm; the
 * complete iterate lands in level 0's u (no sweep stays owed).  Every flag is reset as mgi_start does; the coarse-level graph and the LDS tail
 * are used */
int    mgi_apply_cycle(mg_solver *s);
/* the same for the fp32 cycle of a mixed-precision solver (mg_cg_mixed.c): level 0's fp32 b -> level 0's fp32 u, from the zero guess.  jz != 0:
 * level 0's fp32 tmp holds the first sweep already; mgi_mixed_jz tells whether the cycle can take it (the condition of the mixed iteration) */
int    mgi_apply_cycle_f32(mg_solver *s, int jz);
int    mgi_mixed_jz(const mg_solver *s);
/* the five fine-level fields, the device slot and the reduction workspace of the CG drivers (DEFINED in mg_cg.c, for mg_cg_mixed.c): allocated
 * once; a failure names `who`, the count and the bytes and leaves nothing allocated */
int    mgi_cg_alloc(mg_solver *s, const char *who);
#endif
