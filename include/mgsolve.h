/*
 * mgsolve.h -- host-side C API of the MI355X multigrid V-cycle (the product's own driver).
 *
 * Mirrors the call sequence of the reference driver for `-cycle 0`
 * (src/poisson.c:27-138: SetUpMesh -> SetUpIndices/mapping -> SetUpOperator -> SetUpSolver ->
 *  Assemble -> Solve -> Postprocessing) without the O(N) host index maps and the ~5N scalar
 * MatSetValue calls that make the reference driver infeasible beyond ~4097^2:
 * operators are matrix-free constant stencils, maps are the implicit lexicographic formula.
 * Host code is C99; every device operation goes through the kernel ABI of include/mgk.h.
 *
 * The same objects serve 2-D (the reference's DIMENSION 2) and the 3-D extension.
 * There is no CPU fallback: creating a solver without a HIP device fails with MGK_ENOGPU.
 */
#ifndef MGSOLVE_H
#define MGSOLVE_H
#include "mgk.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MG_KSP_RICHARDSON = 0, MG_KSP_CHEBYSHEV = 1 } mg_ksp_type;
typedef enum { MG_PREC_FP64 = 0, MG_PREC_MIXED = 1 } mg_precision;
typedef enum { MG_PC_JACOBI = 0, MG_PC_LINE_Y = 1, MG_PC_LINE_X = 2, MG_PC_LINE_ALT = 3, MG_PC_RBGS = 4 } mg_pc_type;

/* the bits of mg_config.fuse: one fused pass (or family of passes) each.  The VALUES are ABI: tests, bench.py, the tools and
 * `mgpoisson -mg_fuse N` pass numerals.  "(bit N)" is the name the bit goes by in DESIGN.md, the tests and the profiles. */
typedef enum mg_fuse_bits {
    /* (bit 0) final residual fused with its norm (no rv write) */
    MG_FUSE_RESNORM = 1,
    /* (bit 1) prolongation fused into the first post-smoothing sweep */
    MG_FUSE_PROLONG_SWEEP = 2,
    /* (bit 2) pre-restriction residual fused with the restriction */
    MG_FUSE_RES_RESTRICT = 4,
    /* (bit 3) the residual norm that closes a cycle is evaluated by the kernel that also makes the first pre-smoothing sweep of the
     * next cycle (adopted only if a next cycle runs) */
    MG_FUSE_NORM_SWEEP = 8,
    /* (bit 4; mixed precision) the fp64 correction u += e and the fp64 residual -> fp32 in one pass */
    MG_FUSE_MIXED_CORRECT = 16,
    /* (bit 5) pairs of sweeps in one pass (temporal blocking, levels >= pair_min_n, both precisions) */
    MG_FUSE_PAIRS = 32,
    /* (bit 6, value 64) unassigned: callers pass it (fuse = 127, 63 | 64), so it stays accepted and is ignored */
    /* (bit 7; testing) bit 2 also below 255^3, where two short kernels are quicker */
    MG_FUSE_RES_RESTRICT_SMALL = 128,
    /* (bit 8) the fused residual+restriction also writes the coarse level's first (zero-guess) sweep */
    MG_FUSE_COARSE_ZERO_SWEEP = 256,
    /* (bit 9) the levels that fit in LDS (n <= 15 in 3-D, <= 63 in 2-D) run as ONE kernel per cycle (mgk_tail_cycle_*) */
    MG_FUSE_LDS_TAIL = 512,
    /* (bit 10; fp64, 3-D, full-row shapes n = 127 .. 1023, whole grids and z-slabs) the pass of bit 3 makes the first TWO sweeps of the
     * next cycle (mgk_jacobi2_sumsq_f64 / _slab_f64) and the last pre-smoothing sweep runs inside the restriction's pass
     * (mgk_sweep_residual_restrict_f64 / _slab_f64): the fine level moves 99 instead of 115 B per unknown and cycle */
    MG_FUSE_SWEEP_RESTRICT = 1024,
    /* (bit 11; 3-D whole levels that sweep in pairs: fp32 up to 1023^3, fp64 up to 511^3) a pre-smoothing of >= 3 sweeps from the zero
     * guess starts with ONE pass that makes three of them and reads b alone (mgk_jacobi2_zero_*) */
    MG_FUSE_ZERO_TRIPLE = 2048,
    /* (bit 12; fp64, 3-D, level 0 of 511- / 1023-wide whole grids, v0 = 3) post-smoothing is ONE pass for the prolongation and two
     * sweeps (mgk_prolong_jacobi2_f64); the third sweep is the first stage of the two-sweep pass that evaluates the norm
     * (mgk_jacobi2_sumsq_mid_f64): 91 B per fine unknown and cycle.  The iterate the norm belongs to is not stored; when the
     * iteration stops one more sweep materialises it */
    MG_FUSE_PROLONG_PAIR = 4096,
    /* (bit 13; 2-D, fp64, Richardson, uniform and stretched meshes) THREE sweeps per pass (mgk_jacobi3_2d_*): pre-smoothing from the
     * zero guess in one pass over b, post-smoothing in one pass with the prolongation, and the norm pass of bit 3 makes all three
     * pre-smoothing sweeps of the next cycle: three passes over a level per V(3,3) cycle */
    MG_FUSE_TRIPLE_2D = 8192,
    /* (bit 14; round 3; nranks > 1) bit 12's three passes on z-slabs -- mgk_prolong_jacobi2_slab_f64 (the neighbours' boundary and
     * second planes of u and of the coarse u arrive in two grouped exchanges hidden behind the interior planes),
     * mgk_jacobi2_sumsq_mid_slab_f64, the plain fused residual + restriction: every rank moves 91 instead of 99 B per fine unknown
     * and cycle */
    MG_FUSE_PROLONG_PAIR_SLAB = 16384,
    /* (bit 15, 32768; KSPCHEBYSHEV, fp64, one rank) the smoothings with exactly three steps of 2-D levels run as ONE three-step pass
     * each (mgk_cheby3_2d_*: the passes, swaps and bytes of bit 13's Richardson cycle, coarse-level graph included), and the levels
     * that fit in LDS as one kernel per cycle in 2-D and 3-D with any step counts (mgk_tail_cycle_cheby_f64, with bit 9); off: every
     * step is a launch of its own */
    MG_FUSE_CHEBY = 32768,
    /* bits 0-5 and 8-15: what mg_config.fuse = -1 selected before bit 16 (below) joined it */
    MG_FUSE_DEFAULT = MG_FUSE_RESNORM | MG_FUSE_PROLONG_SWEEP | MG_FUSE_RES_RESTRICT | MG_FUSE_NORM_SWEEP | MG_FUSE_MIXED_CORRECT | MG_FUSE_PAIRS |
                      MG_FUSE_COARSE_ZERO_SWEEP | MG_FUSE_LDS_TAIL | MG_FUSE_SWEEP_RESTRICT | MG_FUSE_ZERO_TRIPLE | MG_FUSE_PROLONG_PAIR |
                      MG_FUSE_TRIPLE_2D | MG_FUSE_PROLONG_PAIR_SLAB | MG_FUSE_CHEBY
} mg_fuse_bits;
/* (bit 16, 65536; fp64, 3-D, one rank, level 0 of 511- / 1023-wide whole grids, v0 = 3; with bits 10 and 12) the pass of bit 12 that makes the
 * owed third post-smoothing sweep and the norm also makes the first TWO pre-smoothing sweeps of the next cycle, three sweeps in one pass
 * (mgk_jacobi3_sumsq_mid_f64, include/mgk_sweep3.h), and the third one runs inside the restriction's pass (bit 10):
 * (P + S1, S2)(S3, N + S1', S2')(S3' + R) = 25 + 24 + 26 = 75 B per fine unknown and cycle instead of 91.  The z-slab path keeps the 91-byte
 * passes.  Same iterates and norms bit for bit.  The same bit (3-D, fp64, one rank, Richardson + point Jacobi, v0 >= 3): where the post-smoothing
 * of a 511- / 1023-wide level outside the coarse-level graph is not made by bit 12 -- level 1 of a 1025^3 solve, level 0 in the last cycle of a
 * call -- the prolongation, its correction and three sweeps run as one pass (mgk_prolong_jacobi3_f64): 25 instead of 49 B per unknown of that
 * level.  The bit and MG_FUSE_AUTO stand beside the enum, whose enumerators and whose
 * MG_FUSE_DEFAULT keep the values they have always had (ABI) */
#define MG_FUSE_TRIPLE_MID 65536
/* what mg_config.fuse = -1 selects: MG_FUSE_DEFAULT and bit 16 */
#define MG_FUSE_AUTO (MG_FUSE_DEFAULT | MG_FUSE_TRIPLE_MID)
/* (bit 17, 131072; not part of MG_FUSE_AUTO: mg_config.fuse = -1 adds it per width, where level 0 has rows of 1024 -- the gate of
 * profiles/triple_norm/README.md is met there and not at rows of 512, where the bit is opt-in.  Where bit 16 runs its 75-byte passes -- fp64, 3-D, one rank, Richardson + point Jacobi,
 * v0 = 3, level 0 a 511- / 1023-wide whole grid outside the coarse-level graph and not feeding it) the 66-byte level of DESIGN.md section 4
 * (xxii): post- and pre-smoothing as two stacked passes and the plain residual + restriction,
 * (P + S1, S2, S3)(N + S1', S2', S3')(R) = 25 + 24 + 17 B per fine unknown and cycle.  Level 0's post-smoothing is the prolongation +
 * three-sweep pass in every cycle, so no sweep is owed and u is the iterate the norm belongs to; the pass that evaluates the norm
 * (mgk_jacobi3_sumsq_f64) makes all three pre-smoothing sweeps of the next cycle.  The closing cycle of a call and a cycle that has no
 * speculative sweeps to adopt keep their passes.  Same iterates bit for bit; the norms are those of the stored iterate, summed per block */
#define MG_FUSE_TRIPLE_NORM 131072

/* options of the reference driver (src/poisson.c:51-59, poisson.in) + the PETSc options that
 * KSPSetFromOptions (src/solver.c:1476,1492,1509) would pick up for the smoother */
typedef struct mg_config {
    int dim;            /* 2 (reference) or 3 (extension) */
    int npts;           /* -npts : points per side INCLUDING the boundary; unknowns per side = npts-2 */
    int levels;         /* -levels (== -grids: one grid per level, the V-cycle case) */
    int v[2];           /* -v v0,v1 : sweeps on levels 0..L-2 / on the coarsest level */
    int maxiter;        /* -iter */
    int ksp_type;       /* -ksp_type richardson|chebyshev */
    double scale;       /* -ksp_richardson_scale (PETSc default 1.0) */
    double emin, emax;  /* -ksp_chebyshev_eigenvalues emin,emax */
    double rtol;        /* stopping factor of src/solver.c:1530; <=0 selects the reference's 1.e-7 */
    int device;         /* HIP device ordinal */
    int precision;      /* mg_precision */
    int rank, nranks;   /* z-slab decomposition over `nranks` GPUs (1: whole grid) */
    int dist_min_n;     /* levels with n >= dist_min_n stay distributed, coarser ones are replicated; <=0: default 255
                         * (below that a slab sweep is shorter than the latency of its halo exchange) */
    int fuse;           /* which fused passes a cycle may use: a mask of mg_fuse_bits (above).  Every bit exists so that tests can run the
                         * unfused path as the reference; which path runs is otherwise decided by what the solver sees (dimension, v0,
                         * ranks).  -1 selects the default set, MG_FUSE_AUTO, and MG_FUSE_TRIPLE_NORM with it in 3-D at npts = 1025 */
    int overlap;        /* nranks > 1: halo of sweep k on the comm stream while sweep k's interior runs; default on (-1) */
    int graph;          /* replay the launch-bound coarse levels as one captured HIP graph; default on (-1) */
    int pair_min_n;     /* levels with n >= pair_min_n run their sweeps two per pass (fuse bit 5); <=0: default 255 (3-D), 2047 (2-D) */
    int slab_chunk;     /* nranks > 1: planes per workgroup of the marching kernels (short blocks let the exchange kernels in beside the
                         * interior launches); <0: default = a quarter of the rank's fine planes, at least 32 (MG_SLAB_CHUNK overrides); 0: the long
                         * streams of a single GPU */
    int mesh;           /* -mesh: 0 uniform; 1 / 2: the reference's meshes stretched in y (src/mesh.c:45-107,165-169), 2-D, one GPU,
                         * Richardson + Jacobi: the operator rows then depend on the grid row (per-row coefficient tables); the same
                         * fused cycle on the row-table forms of its kernels (mgk_*_rowcoef_f64) */
    int pc_type;        /* -pc_type: MG_PC_JACOBI (0, default) point Jacobi; MG_PC_LINE_Y (1) y-line Jacobi: one sweep is u <- u + scale T^-1 (b - A u)
                         * with T the y-tridiagonal part of A, solved exactly in every column (Thomas; the factorisation is the same in every
                         * column, three tables per level made at creation) by a forward and a backward pass (mgk_line_forward_f64 /
                         * mgk_line_backward_f64).  The remedy for the cells of -mesh 1 that are thin in y, where point Jacobi stops smoothing:
                         * the cycle count no longer grows with npts.  2-D, fp64, one rank, Richardson, meshes 0 / 1 / 2, any v and scale;
                         * anything else is refused by mg_solver_create with MGK_EINVAL, and so are mg_solver_fmg*, mg_solver_solve_gmres on
                         * such a solver.  The fuse bits that bake point Jacobi into a pass (1, 3, 5, 8-15) are cleared; bits 0 and 2 stay,
                         * the coarse levels run by launch inside the HIP graph (a line sweep swaps no buffers).
                         * MG_PC_LINE_X (2) x-line Jacobi: the same with T the x-tridiagonal part of A, solved exactly in every row (one table
                         * per level; mgk_xline_forward_f64 / mgk_xline_backward_f64), for a mesh stretched in x.  MG_PC_LINE_ALT (3) alternating
                         * line relaxation: within one smoothing (one KSPSolve of max_it sweeps, counted from 0 in every call) sweep k is a
                         * y-line sweep for even k and an x-line sweep for odd k -- the same number of sweeps as MG_PC_LINE_Y, and a cycle count
                         * independent of npts on meshes 0, 1 and 2.  Both under the conditions of MG_PC_LINE_Y, with
                         * the same refusals.
                         * MG_PC_RBGS (4) red-black Gauss-Seidel: point (i, j) has the colour (i + j) & 1; a sweep updates
                         * colour 0, then colour 1 from the new values, each point by the expression of point Jacobi with `scale` as the
                         * relaxation factor.  It converges at scale 1 (PETSc's default), where the Jacobi-type smoothers need 0.8 or GMRES.
                         * A smoothing of v sweeps is v / 2 passes of two sweeps and one of one sweep if v is odd (mgk_rbgs_2d_f64; with fuse
                         * bit 1 the first post-smoothing pass also prolongs, mgk_prolong_rbgs_2d_f64); every pass swaps u / tmp, an even
                         * number of times per level and cycle.  Conditions and refusals of MG_PC_LINE_Y; line_chunk, xline_chunk and
                         * line_tail must be 0.  Fuse bits 0, 1 and 2 stay, bits 3, 5 and 8-15 are cleared; the coarse levels run by launch
                         * inside the HIP graph */
    int line_tail;      /* (0, default: off) 1: the coarse levels of a line cycle (MG_PC_LINE_Y / _X / _ALT) whose fields fit in LDS run as ONE
                         * kernel per cycle (mgk_tail_cycle_line_f64) instead of two launches per sweep plus the
                         * transfers -- what fuse bit 9 is to point Jacobi.  Bit-identical to the launches it replaces.  The tail starts at
                         * the first level l >= 1 with n <= 63 that is also below every chunk period that applies (n < line_chunk where
                         * the pc has y sweeps, n < xline_chunk where it has x sweeps: the kernel makes plain sweeps only); it needs 2 to 8
                         * such levels and v0 >= 1, otherwise 1 is accepted and the tail stays off (mg_solver_tail_level tells).
                         * Independent of `fuse`: bit 9 stays cleared for the line smoothers, and fuse = 0 with line_tail = 1 still uses the
                         * tail.  Any other value, or 1 with MG_PC_JACOBI: MGK_EINVAL.  (The two chunk periods stay the last
                         * fields of the struct: new options go before them) */
    int xline_chunk;    /* (0, default: off) c > 0, a multiple of 16: every x-line sweep (MG_PC_LINE_X, the odd sweeps of MG_PC_LINE_ALT) solves its
                         * tridiagonal systems in chunks of c columns -- column q c + c - 1 is a separator, the c - 1 columns before it a
                         * chunk; the chunks are solved independently, the n / c separators of a row by their Schur complement, the chunks
                         * corrected by two spike vectors (line_chunk turned by 90 degrees; two more tables of the size
                         * of the x table, three of n / c values per row and a workspace of 4 n / c rows per level) -- so that a pass runs on
                         * n / c + 1 times as many waves: four passes per sweep (mgk_xline_chunk_*_f64) instead of two.  The arithmetic
                         * differs from the plain sweep by rounding (its own definition, tests/xchunkline_reference.py); a level with
                         * n < c keeps the plain sweep.  Independent of line_chunk.  < 0, not a multiple of 16, or > 0 with
                         * MG_PC_JACOBI / MG_PC_LINE_Y: MGK_EINVAL */
    int line_chunk;     /* (0, default: off) c >= 2: every y-line sweep (MG_PC_LINE_Y, the even sweeps of MG_PC_LINE_ALT) solves its tridiagonal
                         * systems in chunks of c rows -- row j c + c - 1 is a separator, the c - 1 rows before it a chunk; the chunks are
                         * solved independently, the n / c separators by their Schur complement, the chunks corrected by two spike
                         * vectors (five more tables of n and three of n / c doubles per level) -- so that a pass
                         * runs on n / c + 1 times as many waves: four passes per sweep (mgk_line_chunk_*_f64) instead of two.  The
                         * arithmetic differs from the plain sweep by rounding (its own definition, tests/chunkline_reference.py); a level
                         * with n < c keeps the plain sweep.  < 0, 1, or > 0 with MG_PC_JACOBI / MG_PC_LINE_X: MGK_EINVAL */
} mg_config;

void mg_config_default(mg_config *cfg);     /* poisson.in defaults + -pc_type jacobi -ksp_richardson_scale 1 */

typedef struct mg_solver mg_solver;

/* communication hooks for nranks > 1 (see mg_comm.h); a solver with nranks == 1 needs none */
struct mg_comm;

int  mg_solver_create(mg_solver **s, const mg_config *cfg, struct mg_comm *comm);
void mg_solver_destroy(mg_solver *s);
const char *mg_last_error(void);

/* levelvecb (src/solver.c:558-620) with Ffunc (src/problem.c:24-28) on the uniform mesh (src/mesh.c:130-195) */
int  mg_solver_set_rhs_problem(mg_solver *s);
/* arbitrary right-hand side: compact lexicographic array of the LOCAL slab (nz_local*ny*nx doubles) */
int  mg_solver_set_rhs_host(mg_solver *s, const double *b_compact);
/* u0 = 0, iteration counter and KSP guess flags back to their initial state (src/solver.c:1512-1523) */
int  mg_solver_reset(mg_solver *s);
/* Solve(): MultigridVcycle (src/solver.c:1414-1575) until ||r|| <= rtol*||b||, divergence, or maxiter */
int  mg_solver_solve(mg_solver *s);
/* exactly `ncycles` more V-cycles from the current state (no stopping test); used by bench.py */
int  mg_solver_cycles(mg_solver *s, int ncycles);
/* full multigrid FMG(nu) (PETSc's -pc_mg_type full) on the current right-hand side: b_l = R b_{l-1} down the levels, v1 sweeps from the
 * zero guess on the coarsest, then on each finer level l: u_l = 0 + P u_{l+1} and nu V-cycles on the levels l .. L-1 from that guess.
 * Leaves the solver as one iteration would (rnorm[0] = ||b||, rnorm[1] = ||b - A u0||, iterations = 1); mg_solver_cycles continues
 * with V-cycles from u0.  One GPU, fp64, Richardson + point Jacobi, uniform mesh, levels >= 2, nu >= 1: anything else returns MGK_EINVAL. */
int  mg_solver_fmg(mg_solver *s, int nu);
/* FMG(nu), then V-cycles under the stop rule of mg_solver_solve; solve_seconds covers both */
int  mg_solver_solve_fmg(mg_solver *s, int nu);
/* Restarted GMRES(restart) with the V-cycle as right preconditioner (PETSc's -ksp_type gmres -pc_type mg -ksp_pc_side right) on the current
 * right-hand side, classical Gram-Schmidt without refinement.  M = one V-cycle from the zero guess, A = the fine-level operator:
 *   x = 0, r = b, beta = ||b||, v_0 = r / beta;
 *   step j: z = M v_j, w = A z, h_i = v_i . w (i <= j), w -= sum h_i v_i, h_{j+1} = ||w||, Givens rotations give the estimate |g_{j+1}| of
 *           ||b - A x_j||, v_{j+1} = w / h_{j+1};
 *   at a stop or after `restart` steps: H y = g, x += M (V y); going on from r = b - A x, beta = ||r||.
 * Stops when the estimate is <= rtol ||b||, after maxiter steps, or under the divergence guard of mg_solver_solve; h_{j+1} = 0 ends it as
 * converged.  On return: the solution is x, level 0's right-hand side is the caller's, iterations = Arnoldi steps (= applications of M
 * less one per restart cycle), rnorm[0] = ||b||, rnorm[k] = the estimate after step k, solve_seconds covers the call; reset + solve
 * then behave as on a fresh solver.  The first call for a restart length allocates restart + 4 fine-level fields (freed by
 * mg_solver_destroy); if they do not fit the error names the restart length and the bytes and nothing stays allocated.
 * One GPU, fp64, Richardson + point Jacobi, any mesh, 2-D and 3-D, 1 <= restart <= MGK_KRYLOV_MAX - 1: anything else returns MGK_EINVAL. */
int  mg_solver_solve_gmres(mg_solver *s, int restart);
/* Conjugate gradients with the V-cycle as preconditioner (PETSc's -ksp_type cg -pc_type mg) on the current right-hand side, for the uniform
 * mesh, where the fine-level operator A and the cycle M (one V-cycle from the zero guess) are both symmetric:
 *   x = 0, r = b, z = M r, p = z, rho = r . z;
 *   step k: q = A p, sigma = p . q, alpha = rho / sigma; x += alpha p, r -= alpha q, rnorm[k] = ||r||;
 *           stop, or z = M r, rho' = r . z, beta = rho' / rho, p = z + beta p, rho = rho'.
 * Every product and sum is rounded separately (no FMA).  Stops when rnorm[k] <= rtol ||b||, after maxiter steps, or under the divergence
 * guard of mg_solver_solve.  A BREAKDOWN -- alpha not finite or <= 0, beta not finite or < 0: M is indefinite, as with an over-relaxed
 * smoother -- ends the iteration like a stop: the return code is 0, the history ends at the last completed step and the solution is that
 * step's x; mg_solver_cg_breakdown tells the step.  On return: the solution is x, level 0's right-hand side is the caller's, iterations =
 * CG steps, rnorm[0] = ||b||, solve_seconds covers the call; reset + solve then behave as on a fresh solver.  ||b|| = 0 or maxiter < 1: the
 * solution is 0, no step.  The first call allocates five fine-level fields whatever the step count (freed by mg_solver_destroy); if they do
 * not fit the error names the count and the bytes and nothing stays allocated.  Per step: one cycle, 96 B per fine unknown in three
 * launches, three host synchronisations.
 * One GPU, fp64 (a mixed-precision solver: mg_solver_solve_cg_mixed), Richardson + point Jacobi, the uniform mesh (mesh == 0; elsewhere use
 * mg_solver_solve_gmres), 2-D and 3-D: anything else returns MGK_EINVAL with a message of its own. */
int  mg_solver_solve_cg(mg_solver *s);
/* the step (1-based) in which the last mg_solver_solve_cg or mg_solver_solve_cg_mixed broke down; 0: it did not */
int  mg_solver_cg_breakdown(const mg_solver *s);
/* The same conjugate gradients in fp64 on a solver created with precision = MG_PREC_MIXED, preconditioned by the fp32 V-cycle its plain
 * iteration runs between two defect corrections: M r = (double) Vcycle32((float) r) from the zero guess.
 *   x = 0, r = b, r32 = (float) r, z32 = Vcycle32(r32), rho = sum r * (double) z32;
 *   step k: p = (double) z32 + beta p, q = A p, sigma = p . q, alpha = rho / sigma; x += alpha p, r -= alpha q, rnorm[k] = ||r||, r32 = (float) r;
 *           stop, or z32 = Vcycle32(r32), rho' = sum r * (double) z32, beta = rho' / rho, rho = rho'.
 * x, r, p, q, A and every sum are fp64, rounded as in mg_solver_solve_cg; (float) rounds to nearest, (double) is exact.  The stop rule, the
 * breakdown semantics (mg_solver_cg_breakdown), what is left in the solution, the right-hand side, rnorm, iterations and solve_seconds,
 * ||b|| = 0 or maxiter < 1, reset + solve afterwards and the five fine-level fields of the first call are those of mg_solver_solve_cg (the two
 * entry points share the fields).  The fp32 cycle is symmetric to about 3e-7 only; at rtol 1e-7 the step counts are those of fp64 CG.  Per step:
 * one fp32 cycle and 92-96 B per fine unknown in three launches, three host synchronisations.
 * A mixed-precision solver (3-D), one GPU, Richardson + point Jacobi, the uniform mesh: anything else returns MGK_EINVAL with a message of its
 * own. */
int  mg_solver_solve_cg_mixed(mg_solver *s);
/* block until every stream of this solver's device is idle */
int  mg_solver_sync(mg_solver *s);

int    mg_solver_iterations(const mg_solver *s);          /* solver->numIter (src/solver.c:1558) */
double mg_solver_bnorm(const mg_solver *s);
/* absolute residual norms rnorm[0..iterations] (src/solver.c:1520,1549) BEFORE the division by rnorm[0] */
const double *mg_solver_rnorm(const mg_solver *s);
double mg_solver_solve_seconds(const mg_solver *s);       /* "Solver walltime" window (src/solver.c:1526,1553) */

int  mg_solver_num_levels(const mg_solver *s);
/* test aid: the kernel context (mgk_ctx *, include/mgk.h) this solver launches on, for mgk_debug_partials / mgk_sync; NULL without a solver */
void *mg_solver_debug_kernel_ctx(mg_solver *s);
/* the first level that runs inside a tail kernel (fuse bit 9, or line_tail with a line smoother): it and every coarser level are one launch
 * per cycle, their fields in LDS; 0: none */
int  mg_solver_tail_level(const mg_solver *s);
/* launches of the prolongation + three-sweep pass (fuse bit 16) on a level since the solver was created */
int  mg_solver_prolong_triple_launches(const mg_solver *s, int level);
/* launches of the norm + three-sweep pass of level 0 (fuse bit 17) since the solver was created */
int  mg_solver_triple_norm_launches(const mg_solver *s);
/* recordings of the coarse-level graph thrown away since the solver was created because the level that feeds it had swapped u / tmp an odd
 * number of times since the recording (0 in every default configuration) */
int  mg_solver_graph_rerecorded(const mg_solver *s);
int  mg_solver_level_n(const mg_solver *s, int level);              /* unknowns per side */
int  mg_solver_level_local_planes(const mg_solver *s, int level, int *z0);
long mg_solver_local_unknowns(const mg_solver *s);
/* smoother point updates of one V-cycle summed over levels (all ranks): sum_l sweeps_l * N_l */
double mg_solver_dof_updates_per_cycle(const mg_solver *s);

/* fine-level solution of the local slab, compact lexicographic (GetSol, src/solver.c:1239-1315) */
int  mg_solver_get_solution(mg_solver *s, double *u_compact);
/* GetError (src/solver.c:1211-1237): {max|e|, sum|e|, sqrt(sum e^2)} against sin(pi x)sin(pi y)[sin(pi z)] */
int  mg_solver_error_norms(mg_solver *s, double err[3]);

/* per-kernel event timing of the fine-level smoother sweeps (bench.py roofline leg) */
int  mg_solver_profile(mg_solver *s, int enable);
int  mg_solver_profile_read(mg_solver *s, double *total_ms, int *launches);
/* the same for one kind of launch: 0 = plain fine-level sweeps, 1 = two-sweeps-in-one-pass launches (in the 75-byte cycle of fuse bit 16: the
 * prolongation + two sweeps pass, the only one left on level 0), 2 = the three-sweep pass of fuse bit 16 / the norm + three-sweep pass of bit 17 */
int  mg_solver_profile_read_kind(mg_solver *s, int kind, double *total_ms, int *launches);

/* integer half of the reference (src/matbuild.c), implicit form */
void mg_get_ranges(int totaln, int procs, int *ranges);             /* matbuild.c:120-144 */
int  mg_grid_n(int npts, int grid);                                 /* matbuild.c:62-66 */
/* one-grid-per-level maps: grid (i,j[,k]) <-> global lexicographic index (matbuild.c:280-309) */
long mg_grid_to_global(int dim, int n, int k, int i, int j);
void mg_global_to_grid(int dim, int n, long idx, int *k, int *i, int *j);
/* plane-aligned slab split used by the multi-GPU path: [z0,z1) of level `level` for `rank` */
int  mg_slab_range(int npts, int levels_dist, int level, int rank, int nranks, int *z0, int *z1);

#ifdef __cplusplus
}
#endif
#endif
