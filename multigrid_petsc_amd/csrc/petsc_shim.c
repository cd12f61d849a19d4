/*
 * petsc_shim.c -- the PETSc Mat/Vec/KSP call surface of include/petscksp.h on the MI355X kernel ABI.
 *
 * What the reference does with PETSc on the `-cycle 0` path (paths relative to /root/reference):
 *   assembles A[l], res[l], pro[l] with MatSetValue            src/solver.c:185-253,1035-1154
 *   fills b[0] with VecSetValue                                src/solver.c:558-620
 *   runs KSPSolve / KSPBuildResidual / MatMult / VecAXPY / VecNorm in the cycle loop   :1530-1550
 *   reads the solution back with VecGetArray                   src/solver.c:1255
 * Here MatAssemblyEnd RECOGNISES the operator families the reference assembles -- constant 5-point rows, 9-entry full
 * weighting rows, <=4-entry bilinear rows, 5-point rows whose coefficients depend on the grid row (-mesh 1/2), and the
 * I-cycle's coupled level operator of several grids (-cycle 1, src/solver.c:255-487) -- and replaces them by matrix-free
 * stencil / transfer operators on the padded device layout; anything else stays an assembled AIJ matrix that is
 * multiplied on the GPU by a generic CSR kernel.  KSP: richardson | chebyshev | preonly with jacobi | none | lu (an exact
 * solve for PCMG's coarsest grid) | mg.  There is no CPU execution path for Mat/Vec/KSP operations (host work happens
 * once per operator: CSR compression, recognition, the dense inverse of a PCLU operator).
 *
 * C99, no HIP: every device operation is a call into include/mgk.h.
 */
#include "petscksp.h"
#include "mgk.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

/* ------------------------------------------------------------------ */
/* global state, errors                                                */
/* ------------------------------------------------------------------ */
static mgk_ctx *G = NULL;
static int g_notice_pc = 0;
static long g_lzstat[16];    /* lazy temporaries: [0] residual+restriction fused, [1] prolongation fused into a sweep, [2..4] deferred values that were
                              * computed after all (residual, prolongation, correction), [5] deferred values overwritten unread; ...; [14] three-sweep
                              * passes (mgk_jacobi3_2d_*, mgk_prolong_jacobi3_2d_f64), [15] two-sweep passes of KSPSolve (mgk_jacobi2_2d_f64) */

static void tc_shutdown(void);       /* the tail recorder's logs (below) */
static void die(const char *what) {
    fprintf(stderr, "[mgpetsc] FATAL: %s (kernel layer: %s)\n", what, mgk_last_error());
    exit(86);
}
#define DEV(call) do { if ((call) != 0) die(#call); } while (0)
#define UNSUPPORTED(name) do { fprintf(stderr, "[mgpetsc] FATAL: %s is outside the V-cycle hot path and is not implemented " \
    "by this drop-in (see INTEGRATION.md)\n", name); exit(87); } while (0)

static void need_ctx(void) {
    if (!G) { fprintf(stderr, "[mgpetsc] FATAL: PetscInitialize() has not been called\n"); exit(85); }
}

/* ------------------------------------------------------------------ */
/* options database: src/poisson.c:29,51-59; poisson.in                */
/* ------------------------------------------------------------------ */
typedef struct { char *key, *val; } opt_t;
static opt_t *g_opt = NULL;
static int g_nopt = 0, g_capopt = 0;

static void opt_set(const char *key, const char *val) {
    for (int q = 0; q < g_nopt; q++)
        if (!strcmp(g_opt[q].key, key)) { free(g_opt[q].val); g_opt[q].val = strdup(val ? val : ""); return; }
    if (g_nopt == g_capopt) { g_capopt = g_capopt ? 2 * g_capopt : 32; g_opt = (opt_t *)realloc(g_opt, sizeof(opt_t) * (size_t)g_capopt); }
    g_opt[g_nopt].key = strdup(key); g_opt[g_nopt].val = strdup(val ? val : ""); g_nopt++;
}
static const char *opt_get(const char *key) {
    for (int q = 0; q < g_nopt; q++) if (!strcmp(g_opt[q].key, key)) return g_opt[q].val;
    return NULL;
}
static int is_key(const char *t) {      /* "-name": a dash followed by a letter (so "-1" stays a value) */
    return t && t[0] == '-' && ((t[1] >= 'a' && t[1] <= 'z') || (t[1] >= 'A' && t[1] <= 'Z') || t[1] == '_');
}
static void opt_tokens(char **tok, int n) {
    for (int q = 0; q < n; q++) {
        if (!is_key(tok[q])) continue;
        if (q + 1 < n && !is_key(tok[q + 1])) { opt_set(tok[q], tok[q + 1]); q++; }
        else opt_set(tok[q], "");
    }
}
static void opt_file(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) return;                              /* PETSc also treats a missing options file as empty */
    char line[1024];
    char *tok[4096]; int n = 0;
    while (fgets(line, sizeof(line), f)) {
        char *hash = strchr(line, '#');
        if (hash) *hash = 0;
        for (char *t = strtok(line, " \t\r\n"); t && n < 4096; t = strtok(NULL, " \t\r\n")) tok[n++] = strdup(t);
    }
    fclose(f);
    opt_tokens(tok, n);
    for (int q = 0; q < n; q++) free(tok[q]);
}

PetscErrorCode PetscInitialize(int *argc, char ***argv, const char file[], const char help[]) {
    (void)help;
    if (file) opt_file(file);
    if (argc && argv && *argc > 1) opt_tokens(*argv + 1, *argc - 1);      /* command line overrides the file */
    if (!G) {
        int dev = 0;
        const char *e = getenv("MGPETSC_DEVICE");
        if (e) dev = atoi(e);
        if (mgk_ctx_create(&G, dev) != 0) {
            fprintf(stderr, "[mgpetsc] FATAL: cannot create a HIP context on device %d: %s\n"
                            "          this PETSc-surface drop-in has no CPU fallback.\n", dev, mgk_last_error());
            exit(84);
        }
    }
    return 0;
}
PetscErrorCode PetscFinalize(void) {
    if (getenv("MGPETSC_LAZY_STATS"))
        printf("[mgpetsc] lazy temporaries: %ld residual+restriction passes, %ld prolongation sweeps fused; computed after all: %ld residuals, "
               "%ld prolongations, %ld corrections; %ld dropped unread; %ld zero-guess sweeps out of the restriction's pass; %ld norm passes that store r and make the next sweep, %ld of those sweeps adopted; "
               "%ld norm passes that left r deferred, %ld of those residuals followed the old iterate into the work vector; "
               "%ld coarse sub-cycles run as ONE tail launch, %ld recordings replayed call by call, %ld times their unread intermediates were computed after all; "
               "%ld three-sweep passes, %ld two-sweep passes of KSPSolve\n",
               g_lzstat[0], g_lzstat[1], g_lzstat[2], g_lzstat[3], g_lzstat[4], g_lzstat[5], g_lzstat[7], g_lzstat[6], g_lzstat[8], g_lzstat[9], g_lzstat[10],
               g_lzstat[11], g_lzstat[12], g_lzstat[13], g_lzstat[14], g_lzstat[15]);
    tc_shutdown();
    if (G) { mgk_ctx_destroy(G); G = NULL; }
    for (int q = 0; q < g_nopt; q++) { free(g_opt[q].key); free(g_opt[q].val); }
    free(g_opt); g_opt = NULL; g_nopt = g_capopt = 0;
    return 0;
}
static const char *opt_lookup(const char pre[], const char name[]) {
    if (pre && pre[0]) {
        char k[256];
        snprintf(k, sizeof(k), "-%s%s", pre, name + 1);
        const char *v = opt_get(k);
        if (v) return v;
        return NULL;
    }
    return opt_get(name);
}
PetscErrorCode PetscOptionsGetInt(void *o, const char pre[], const char name[], PetscInt *iv, PetscBool *set) {
    (void)o;
    const char *v = opt_lookup(pre, name);
    if (v && v[0]) { *iv = (PetscInt)strtol(v, NULL, 10); if (set) *set = PETSC_TRUE; }
    else if (set) *set = PETSC_FALSE;            /* absent: the variable is left untouched (src/poisson.c:38-41) */
    return 0;
}
PetscErrorCode PetscOptionsGetReal(void *o, const char pre[], const char name[], PetscReal *dv, PetscBool *set) {
    (void)o;
    const char *v = opt_lookup(pre, name);
    if (v && v[0]) { *dv = strtod(v, NULL); if (set) *set = PETSC_TRUE; }
    else if (set) *set = PETSC_FALSE;
    return 0;
}
PetscErrorCode PetscOptionsGetIntArray(void *o, const char pre[], const char name[], PetscInt iv[], PetscInt *nmax, PetscBool *set) {
    (void)o;
    const char *v = opt_lookup(pre, name);
    if (!v || !v[0]) { if (set) *set = PETSC_FALSE; *nmax = 0; return 0; }
    int n = 0;
    const char *p = v;
    while (*p && n < *nmax) {
        char *end;
        long x = strtol(p, &end, 10);
        if (end == p) break;
        iv[n++] = (PetscInt)x;
        p = end;
        while (*p == ',' || *p == ' ') p++;
    }
    *nmax = n;
    if (set) *set = PETSC_TRUE;
    return 0;
}
PetscErrorCode PetscOptionsSetValue(void *o, const char name[], const char value[]) { (void)o; opt_set(name, value); return 0; }

PetscErrorCode PetscPrintf(MPI_Comm comm, const char format[], ...) {
    (void)comm;
    va_list ap; va_start(ap, format); vfprintf(stdout, format, ap); va_end(ap);
    return 0;
}
PetscErrorCode PetscSynchronizedPrintf(MPI_Comm comm, const char format[], ...) {
    (void)comm;
    va_list ap; va_start(ap, format); vfprintf(stdout, format, ap); va_end(ap);
    return 0;
}
PetscErrorCode PetscSynchronizedFlush(MPI_Comm comm, FILE *fd) { (void)comm; fflush(fd ? fd : stdout); return 0; }
PetscErrorCode PetscLogStageRegister(const char name[], PetscLogStage *stage) { (void)name; if (stage) *stage = 1; return 0; }
PetscErrorCode PetscLogStagePush(PetscLogStage stage) { (void)stage; return 0; }
PetscErrorCode PetscLogStagePop(void) { return 0; }

struct _p_PetscViewer { int kind; };
static struct _p_PetscViewer g_viewer_stdout = {0}, g_viewer_draw = {1};
PetscViewer PETSC_VIEWER_STDOUT_(MPI_Comm comm) { (void)comm; return &g_viewer_stdout; }
PetscViewer PETSC_VIEWER_DRAW_(MPI_Comm comm) { (void)comm; return &g_viewer_draw; }

/* ---- MPI: one process, one GPU ---- */
int MPI_Comm_size(MPI_Comm comm, int *size) { (void)comm; *size = 1; return 0; }
int MPI_Comm_rank(MPI_Comm comm, int *rank) { (void)comm; *rank = 0; return 0; }
double MPI_Wtime(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec + 1e-9 * t.tv_nsec;
}
int MPI_Send(const void *b, int c, MPI_Datatype t, int d, int tag, MPI_Comm comm) {
    (void)b; (void)c; (void)t; (void)d; (void)tag; (void)comm;
    UNSUPPORTED("MPI_Send (more than one rank)");
    return 1;
}
int MPI_Recv(void *b, int c, MPI_Datatype t, int s, int tag, MPI_Comm comm, MPI_Status *st) {
    (void)b; (void)c; (void)t; (void)s; (void)tag; (void)comm; (void)st;
    UNSUPPORTED("MPI_Recv (more than one rank)");
    return 1;
}

/* ------------------------------------------------------------------ */
/* Vec                                                                 */
/* ------------------------------------------------------------------ */
#define MGP_LU_MAX 1024     /* unknowns the exact (PCLU) solve accepts: PCMG's coarsest grid */
#define MGP_MAXG 8          /* grids in one level the matrix-free level operator handles (more: assembled AIJ) */
struct _p_Vec {
    PetscInt n;             /* logical length */
    int padded;             /* 1: grid field in the padded layout `g`; 0: flat array of n doubles;
                             * 2: the `ng` grid fields `gg[0] | gg[1] | ...` back to back, finest first (vectors of the I-cycle's
                             *    several-grids-in-one-level operator); field q starts at goff[q] */
    mgk_geom g;
    int ng; mgk_geom gg[MGP_MAXG]; long goff[MGP_MAXG + 1];
    int lz;                 /* a value that has not been computed yet (lazy temporaries, below): LZ_* */
    struct _p_Mat *lz_A, *lz_A2; struct _p_Vec *lz_b, *lz_x;
    struct _p_KSP *lz_ksp;  /* LZ_RESIDUAL made by KSPBuildResidual: the solver whose next sweep the norm pass can make (below) */
    unsigned long ver;      /* bumped by every write to the vector's value */
    long nalloc;            /* doubles on the device */
    double *dev;
    double *host;           /* compact lexicographic mirror (VecSetValue staging / VecGetArray) */
    int host_dirty;         /* host holds newer values than the device */
    PetscInt ranges[2];
};

static Vec vec_new(PetscInt n, const mgk_geom *g) {
    need_ctx();
    Vec v = (Vec)calloc(1, sizeof(*v));
    v->n = n;
    if (g) { v->padded = 1; v->g = *g; v->nalloc = g->total; }
    else { v->padded = 0; v->nalloc = ((long)n + 15) / 16 * 16; if (v->nalloc < 16) v->nalloc = 16; }
    void *p = NULL;
    DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)v->nalloc));
    v->dev = (double *)p;
    v->ranges[0] = 0; v->ranges[1] = n;
    return v;
}
/* composite of grid fields: every part keeps the padded layout the stencil / transfer kernels work on, the flat BLAS-1
 * kernels run over the whole allocation (ghosts are zero and stay zero) */
static Vec vec_newg(int ng, const mgk_geom *gg) {
    need_ctx();
    Vec v = (Vec)calloc(1, sizeof(*v));
    v->padded = 2; v->ng = ng; v->g = gg[0];
    long n = 0, tot = 0;
    for (int q = 0; q < ng; q++) { v->gg[q] = gg[q]; v->goff[q] = tot; tot += gg[q].total; n += (long)gg[q].nx * gg[q].ny; }
    v->goff[ng] = tot;
    v->n = (PetscInt)n; v->nalloc = tot;
    void *p = NULL;
    DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)v->nalloc));
    v->dev = (double *)p;
    v->ranges[0] = 0; v->ranges[1] = v->n;
    return v;
}
static void vec_upload(Vec v) {          /* host mirror -> device */
    if (!v->host) return;
    if (!v->padded) { DEV(mgk_h2d(G, v->dev, v->host, sizeof(double) * (size_t)v->n)); }
    else {
        void *tmp = NULL;
        DEV(mgk_malloc(G, &tmp, sizeof(double) * (size_t)v->n));
        DEV(mgk_h2d(G, tmp, v->host, sizeof(double) * (size_t)v->n));
        if (v->padded == 2) {
            long o = 0;
            for (int q = 0; q < v->ng; q++) { DEV(mgk_pack_f64(G, &v->gg[q], (const double *)tmp + o, v->dev + v->goff[q], NULL)); o += (long)v->gg[q].nx * v->gg[q].ny; }
        } else DEV(mgk_pack_f64(G, &v->g, (const double *)tmp, v->dev, NULL));
        DEV(mgk_sync(G, NULL));
        mgk_free(G, tmp);
    }
    v->host_dirty = 0;
}
static void vec_download(Vec v) {        /* device -> host mirror */
    if (!v->host) v->host = (double *)malloc(sizeof(double) * (size_t)(v->n > 0 ? v->n : 1));
    if (!v->padded) { DEV(mgk_d2h(G, v->host, v->dev, sizeof(double) * (size_t)v->n)); }
    else {
        void *tmp = NULL;
        DEV(mgk_malloc(G, &tmp, sizeof(double) * (size_t)v->n));
        if (v->padded == 2) {
            long o = 0;
            for (int q = 0; q < v->ng; q++) { DEV(mgk_unpack_f64(G, &v->gg[q], v->dev + v->goff[q], (double *)tmp + o, NULL)); o += (long)v->gg[q].nx * v->gg[q].ny; }
        } else DEV(mgk_unpack_f64(G, &v->g, v->dev, (double *)tmp, NULL));
        DEV(mgk_d2h(G, v->host, tmp, sizeof(double) * (size_t)v->n));
        mgk_free(G, tmp);
    }
}
/* ---- lazy temporaries --------------------------------------------------------------------------------------------------
 * The reference's cycle hands every intermediate result to the next PETSc call through a vector (src/solver.c:1531-1546):
 *   KSPBuildResidual(ksp, NULL, rv, &r); MatMult(res, r, b_coarse)          -- r is read once, by the restriction
 *   MatMult(pro, u_coarse, rv); VecAXPY(u, 1.0, rv); KSPSolve(ksp, b, u)    -- rv is read once, the corrected u is read by the sweep
 * Executed call by call that is 5 passes over the level and 7 launches where the fused kernels of the own driver need 2 passes and
 * 2 launches (b_c = R(b - A u) in one pass; u' = J(u + P u_c) in one pass).  So three results are DEFERRED:
 *   LZ_RESIDUAL  v = b - A x            (MatResidual / KSPBuildResidual on a stencil operator)
 *   LZ_PROLONG   v = P u_c              (MatMult with a recognised prolongation)
 *   LZ_ADDP      v = v + P u_c          (VecAXPY(v, 1.0, rv) with rv = LZ_PROLONG; the device still holds the old v)
 *   LZ_RR        v = R (b - A x)        (MatMult(restriction, r) of an LZ_RESIDUAL r: the Richardson KSPSolve from the zero guess that
 *                                        follows on the coarse level gets its first sweep out of the same pass, mgk_residual_restrict_2d's uc0)
 * and three consumers take them as they are: MatMult(restriction, r) of an LZ_RESIDUAL r runs the fused residual + restriction,
 * VecAXPY(u, 1, rv) of an LZ_PROLONG rv makes u LZ_ADDP, KSPSolve from the guess u of an LZ_ADDP u makes its first sweep with the
 * fused prolongation.  PETSc's semantics are kept for every other use: ANY read of a deferred vector computes it first (vdev ->
 * lz_settle), ANY write to a vector first computes the deferred vectors that depend on it (lz_before_write), destroying an operand
 * likewise.  A deferred vector that is overwritten before anyone reads it is never computed -- which is what happens to r and rv in
 * the reference's loop.  MGPETSC_LAZY=0 switches the whole mechanism off (every call executes at once, as before). */
enum { LZ_NONE = 0, LZ_RESIDUAL = 1, LZ_PROLONG = 2, LZ_ADDP = 3, LZ_RR = 4,
       LZ_TAIL = 5 };      /* written by a recorded (not yet executed) coarse sub-cycle, or an unread intermediate of one that ran as ONE tail launch (below: tail capture) */
#define LZ_MAX 128
static void tc_settle(Vec v);                      /* a LZ_TAIL value is needed: the recording is replayed / the intermediates are computed */
static void tc_dropped(Vec v);                     /* a LZ_TAIL intermediate was overwritten unread */
static int tc_recording_has(Vec v);
static void tc_input_changing(Vec v, int full);    /* the right-hand side of a finished sub-cycle is about to be overwritten */
static void tc_mat_changing(struct _p_Mat *A);
static int tc_axpy(Vec y, double a, Vec x);        /* the three calls below and KSPSolve ask the recorder first: 1 = absorbed */
static int tc_mult(struct _p_Mat *A, Vec x, Vec y);
static int tc_resid(struct _p_Mat *A, Vec b, Vec x, Vec r);
static int g_tc_off = 0;                           /* > 0: no recording (inside PCMG's own cycle, while a recording is replayed) */
static Vec g_lz[LZ_MAX];
static int g_nlz = 0, g_lazy = -1;
static unsigned long g_mat_epoch = 0;      /* bumped when any matrix changes or dies and when any vector dies: speculative sweeps made before are void */
static int lazy_on(void) { if (g_lazy < 0) { const char *e = getenv("MGPETSC_LAZY"); g_lazy = (e && e[0] >= '0' && e[0] <= '9') ? atoi(e) : 1; } return g_lazy; }   /* 2: b_c not deferred (measurement aid) */
static void lz_settle(Vec v);
static void lz_drop(Vec v) {                       /* forget v's deferred value (it is being overwritten / has been consumed) */
    if (!v->lz) return;
    if (v->lz == LZ_TAIL) tc_dropped(v);
    v->lz = LZ_NONE; v->lz_A = v->lz_A2 = NULL; v->lz_b = v->lz_x = NULL; v->lz_ksp = NULL;
    for (int q = 0; q < g_nlz; q++) if (g_lz[q] == v) { g_lz[q] = g_lz[--g_nlz]; break; }
}
static void lz_register(Vec v, int kind, struct _p_Mat *A, Vec b, Vec x) {
    if (g_nlz == LZ_MAX) lz_settle(g_lz[0]);
    v->lz = kind; v->lz_A = A; v->lz_b = b; v->lz_x = x;
    g_lz[g_nlz++] = v;
}
/* before v's value changes: compute whatever is defined in terms of the current v; full: v is overwritten entirely, its own
 * deferred value is dead, otherwise it is computed first */
static void lz_before_write(Vec v, int full) {
    if (v->lz == LZ_TAIL && tc_recording_has(v)) tc_settle(v);      /* a write from outside the pattern: the recording is executed first */
    /* tc_input_changing may hand v's buffer to a finished log and continue v on a spare one: whatever else is defined in terms of v (not the
     * log's own ghosts, which follow the buffer) is computed while v still has it -- a P v deferred by MatMult(pro) was formed from the spare */
    for (int q = 0; q < g_nlz; ) {
        Vec L = g_lz[q];
        if (L != v && L->lz != LZ_TAIL && (L->lz_b == v || L->lz_x == v)) { lz_settle(L); q = 0; } else q++;
    }
    tc_input_changing(v, full);
    for (int q = 0; q < g_nlz; ) {
        Vec L = g_lz[q];
        if (L != v && (L->lz_b == v || L->lz_x == v)) { lz_settle(L); q = 0; } else q++;
    }
    if (v->lz) { if (full) { g_lzstat[5]++; lz_drop(v); } else lz_settle(v); }
    v->ver++;
}
static void lz_before_mat_change(struct _p_Mat *A) {
    g_mat_epoch++;
    tc_mat_changing(A);
    for (int q = 0; q < g_nlz; ) { if (g_lz[q]->lz_A == A || g_lz[q]->lz_A2 == A) { lz_settle(g_lz[q]); q = 0; } else q++; }
}
static double *vdev(Vec v) { if (v->lz) lz_settle(v); if (v->host_dirty) vec_upload(v); return v->dev; }
static int same_layout(Vec a, Vec b) {
    if (a->n != b->n || a->padded != b->padded) return 0;
    if (a->padded == 2 && a->ng != b->ng) return 0;         /* (same finest grid, same count: same chain of grids) */
    if (a->padded) return a->g.dim == b->g.dim && a->g.nx == b->g.nx && a->g.ny == b->g.ny && a->g.nz == b->g.nz;
    return 1;
}
static void need_same(Vec a, Vec b, const char *who) {
    if (!same_layout(a, b)) { fprintf(stderr, "[mgpetsc] FATAL: %s: vectors of different size/layout\n", who); exit(88); }
}

PetscErrorCode VecCreateSeq(MPI_Comm comm, PetscInt n, Vec *v) { (void)comm; *v = vec_new(n, NULL); return 0; }
PetscErrorCode VecDuplicate(Vec v, Vec *nv) { *nv = v->padded == 2 ? vec_newg(v->ng, v->gg) : vec_new(v->n, v->padded ? &v->g : NULL); return 0; }
PetscErrorCode VecDestroy(Vec *v) {
    if (!v || !*v) return 0;
    lz_before_write(*v, 1);                                  /* deferred vectors that read *v are computed now */
    g_mat_epoch++;                                           /* a speculative sweep that names *v is void (the address may be reused) */
    if (G) mgk_free(G, (*v)->dev);
    free((*v)->host); free(*v); *v = NULL;
    return 0;
}
PetscErrorCode VecGetSize(Vec v, PetscInt *n) { *n = v->n; return 0; }
PetscErrorCode VecGetLocalSize(Vec v, PetscInt *n) { *n = v->n; return 0; }
PetscErrorCode VecGetOwnershipRange(Vec v, PetscInt *lo, PetscInt *hi) { if (lo) *lo = 0; if (hi) *hi = v->n; return 0; }
PetscErrorCode VecGetOwnershipRanges(Vec v, const PetscInt *ranges[]) { *ranges = v->ranges; return 0; }
PetscErrorCode VecSetValue(Vec v, PetscInt row, PetscScalar value, InsertMode mode) {
    if (row < 0) return 0;                                   /* PETSc ignores negative indices */
    if (row >= v->n) { fprintf(stderr, "[mgpetsc] FATAL: VecSetValue: row %d out of range %d\n", row, v->n); exit(88); }
    if (!v->host_dirty) { (void)vdev(v); lz_before_write(v, 0); vec_download(v); v->host_dirty = 1; }      /* stage on the current values */
    if (mode == ADD_VALUES) v->host[row] += value; else v->host[row] = value;
    return 0;
}
PetscErrorCode VecAssemblyBegin(Vec v) { (void)v; return 0; }
PetscErrorCode VecAssemblyEnd(Vec v) { if (v->host_dirty) vec_upload(v); return 0; }
PetscErrorCode VecSet(Vec v, PetscScalar a) {
    lz_before_write(v, 1);
    v->host_dirty = 0;
    if (a == 0.0) { DEV(mgk_memset0(G, v->dev, sizeof(double) * (size_t)v->nalloc, NULL)); return 0; }
    if (!v->padded) { DEV(mgk_flat_fill(G, v->n, a, v->dev, NULL)); return 0; }
    /* padded: only the interior may be non-zero */
    if (!v->host) v->host = (double *)malloc(sizeof(double) * (size_t)v->n);
    for (PetscInt q = 0; q < v->n; q++) v->host[q] = a;
    vec_upload(v);
    return 0;
}
PetscErrorCode VecCopy(Vec x, Vec y) {
    need_same(x, y, "VecCopy");
    if (x == y) return 0;
    (void)vdev(x);
    lz_before_write(y, 1);
    y->host_dirty = 0;
    DEV(mgk_d2d(G, y->dev, vdev(x), sizeof(double) * (size_t)x->nalloc, NULL));
    return 0;
}
PetscErrorCode VecScale(Vec v, PetscScalar a) { lz_before_write(v, 0); DEV(mgk_flat_scale(G, v->nalloc, a, vdev(v), NULL)); return 0; }
PetscErrorCode VecAXPY(Vec y, PetscScalar a, Vec x) {       /* y = y + a x  (src/solver.c:1517,1541) */
    need_same(x, y, "VecAXPY");
    if (tc_axpy(y, a, x)) return 0;
    if (x->lz == LZ_PROLONG && a == 1.0 && x != y && y != x->lz_x && y->padded == 1 && lazy_on()) {
        /* u += P u_c with P u_c not computed yet (src/solver.c:1540-1541): u's correction is deferred in turn -- the KSPSolve that
         * follows makes its first sweep on u + P u_c directly; anything else that touches u first runs mgk_prolong_add */
        struct _p_Mat *P = x->lz_A; Vec uc = x->lz_x;
        (void)vdev(y);                                       /* y itself concrete and on the device */
        lz_before_write(y, 0);
        lz_register(y, LZ_ADDP, P, NULL, uc);
        return 0;
    }
    (void)vdev(x);
    lz_before_write(y, 0);
    DEV(mgk_flat_axpy(G, y->nalloc, a, vdev(x), vdev(y), NULL));
    return 0;
}
PetscErrorCode VecAYPX(Vec y, PetscScalar a, Vec x) {       /* y = x + a y */
    need_same(x, y, "VecAYPX");
    (void)vdev(x);
    lz_before_write(y, 0);
    DEV(mgk_flat_aypx(G, y->nalloc, a, vdev(x), vdev(y), NULL));
    return 0;
}
PetscErrorCode VecAXPBYPCZ(Vec z, PetscScalar a, PetscScalar b, PetscScalar c, Vec x, Vec y) {
    need_same(x, z, "VecAXPBYPCZ"); need_same(y, z, "VecAXPBYPCZ");
    (void)vdev(x); (void)vdev(y);
    lz_before_write(z, 0);
    DEV(mgk_flat_axpbypcz(G, z->nalloc, a, b, c, vdev(x), vdev(y), vdev(z), NULL));
    return 0;
}
static int norm_of_deferred_residual(Vec r, double *ss);
PetscErrorCode VecDot(Vec x, Vec y, PetscScalar *val) {
    need_same(x, y, "VecDot");
    DEV(mgk_flat_dot(G, x->nalloc, vdev(x), vdev(y), val, NULL));
    return 0;
}
PetscErrorCode VecTDot(Vec x, Vec y, PetscScalar *val) { return VecDot(x, y, val); }
PetscErrorCode VecNorm(Vec x, NormType type, PetscReal *val) {     /* src/solver.c:1512,1518,1546 */
    if (type != NORM_2 && type != NORM_FROBENIUS) UNSUPPORTED("VecNorm with a norm other than NORM_2");
    double ss;
    if (x->lz == LZ_RESIDUAL && x->lz_ksp && norm_of_deferred_residual(x, &ss)) { *val = sqrt(ss); return 0; }
    DEV(mgk_flat_dot(G, x->nalloc, vdev(x), vdev(x), &ss, NULL));
    *val = sqrt(ss);
    return 0;
}
PetscErrorCode VecGetArray(Vec v, PetscScalar **a) {       /* src/solver.c:1255 */
    if (!v->host_dirty) { (void)vdev(v); lz_before_write(v, 0); vec_download(v); }
    v->host_dirty = 1;                                      /* the caller may write through the pointer */
    *a = v->host;
    return 0;
}
PetscErrorCode VecRestoreArray(Vec v, PetscScalar **a) { if (a) *a = NULL; if (v->host_dirty) vec_upload(v); return 0; }
PetscErrorCode VecView(Vec v, PetscViewer viewer) {
    (void)viewer;
    (void)vdev(v);
    vec_download(v);
    for (PetscInt q = 0; q < v->n; q++) printf("%g\n", v->host[q]);
    return 0;
}
PetscErrorCode VecGetSubVector(Vec v, IS is, Vec *sub) { (void)v; (void)is; (void)sub; UNSUPPORTED("VecGetSubVector"); return 1; }
PetscErrorCode VecRestoreSubVector(Vec v, IS is, Vec *sub) { (void)v; (void)is; (void)sub; UNSUPPORTED("VecRestoreSubVector"); return 1; }
PetscErrorCode ISCreateGeneral(MPI_Comm c, PetscInt n, const PetscInt idx[], PetscCopyMode m, IS *is) {
    (void)c; (void)n; (void)idx; (void)m; (void)is; UNSUPPORTED("ISCreateGeneral (delayed cycles)"); return 1;
}
PetscErrorCode ISDestroy(IS *is) { if (is) *is = NULL; return 0; }
PetscErrorCode ISView(IS is, PetscViewer v) { (void)is; (void)v; return 0; }

/* ------------------------------------------------------------------ */
/* Mat                                                                 */
/* ------------------------------------------------------------------ */
enum { MAT_GENERIC = 0, MAT_STENCIL = 1, MAT_RESTRICT = 2, MAT_PROLONG = 3, MAT_STENCIL_ROW = 4, MAT_LEVELG = 5 };
struct _p_Mat {
    PetscInt m, n;
    int *crow, *ccol; double *cval; long cnz, ccap;     /* MatSetValue stash (COO, insertion order) */
    int assembled;
    long *rowptr; int *col; double *val; long nz;        /* host CSR after assembly */
    int kind;
    mgk_geom gf, gc;                                     /* STENCIL: gf; RESTRICT/PROLONG: fine gf, coarse gc */
    int grow_ok, gcol_ok; mgk_geom grow, gcol;           /* GENERIC on n^2 index spaces (n odd): row / column vectors stay padded grid fields */
    double coef[7];
    int ng; mgk_geom gg[MGP_MAXG]; long goff[MGP_MAXG + 1];   /* LEVELG: the grids of the level, finest first, and their offsets in a vector */
    double coefg[MGP_MAXG][5];                           /*         A_g */
    double *h_wtab[MGP_MAXG][MGP_MAXG], *d_wtab[MGP_MAXG][MGP_MAXG];   /*  [g1][g0], g1 < g0: A_g1 P^(g0-g1) cut to P's window, (2S-1)^2 weights by window offset */
    long *d_rowptr; int *d_col; double *d_val; double *d_dinv;   /* device CSR (generic), lazily built */
    long d_dinv_len;
    double *h_ctab, *h_dtab;                             /* STENCIL_ROW: per-grid-row coefficients (n x 5) and 1/diag (n) */
    double *d_ctab, *d_dtab, *d_ones;
    int dev_stale;
    double *d_inv, *d_c1, *d_c2; int inv_stale;         /* PCLU: dense inverse (m x m, row-major) and two compact work arrays */
    Vec work;
};

PetscErrorCode MatCreateAIJ(MPI_Comm comm, PetscInt m, PetscInt n, PetscInt M, PetscInt N, PetscInt d_nz,
                            const PetscInt d_nnz[], PetscInt o_nz, const PetscInt o_nnz[], Mat *A) {
    (void)comm; (void)d_nnz; (void)o_nz; (void)o_nnz;
    need_ctx();
    Mat a = (Mat)calloc(1, sizeof(*a));
    a->m = m >= 0 ? m : M; a->n = n >= 0 ? n : N;
    a->ccap = (long)a->m * (d_nz > 0 ? d_nz : 8) + 16;
    a->crow = (int *)malloc(sizeof(int) * (size_t)a->ccap);
    a->ccol = (int *)malloc(sizeof(int) * (size_t)a->ccap);
    a->cval = (double *)malloc(sizeof(double) * (size_t)a->ccap);
    *A = a;
    return 0;
}
PetscErrorCode MatSetValue(Mat A, PetscInt row, PetscInt col, PetscScalar value, InsertMode mode) {
    (void)mode;                                          /* the reference only uses ADD_VALUES on fresh matrices */
    if (row < 0 || col < 0) return 0;
    if (A->assembled) UNSUPPORTED("MatSetValue after MatAssemblyEnd");
    if (A->cnz == A->ccap) {
        A->ccap = A->ccap * 2;
        A->crow = (int *)realloc(A->crow, sizeof(int) * (size_t)A->ccap);
        A->ccol = (int *)realloc(A->ccol, sizeof(int) * (size_t)A->ccap);
        A->cval = (double *)realloc(A->cval, sizeof(double) * (size_t)A->ccap);
    }
    A->crow[A->cnz] = row; A->ccol[A->cnz] = col; A->cval[A->cnz] = value; A->cnz++;
    return 0;
}
PetscErrorCode MatAssemblyBegin(Mat A, MatAssemblyType t) { (void)A; (void)t; return 0; }

/* COO -> CSR: rows in ascending column order, duplicates accumulated in insertion order */
static void mat_compress(Mat A) {
    const long m = A->m, nz = A->cnz;
    {   /* the reference fills row after row, every row in ascending column order, no entry twice (src/solver.c:227-251, :1071-1145): then the
         * staged (column, value) arrays ARE the CSR arrays -- one checking pass instead of a counting sort, a sort per row and three copies
         * (MatAssemblyEnd is a third of the reference's set-up time at 4097^2).  Anything else takes the general path below. */
        int sorted = nz > 0;
        for (long q = 1; q < nz && sorted; q++)
            if (A->crow[q] < A->crow[q - 1] || (A->crow[q] == A->crow[q - 1] && A->ccol[q] <= A->ccol[q - 1])) sorted = 0;
        if (sorted && A->crow[0] >= 0 && A->crow[nz - 1] < m) {
            A->rowptr = (long *)calloc((size_t)m + 1, sizeof(long));
            for (long q = 0; q < nz; q++) A->rowptr[A->crow[q] + 1]++;
            for (long r = 0; r < m; r++) A->rowptr[r + 1] += A->rowptr[r];
            A->col = A->ccol; A->val = A->cval; A->nz = nz;
            free(A->crow); A->crow = A->ccol = NULL; A->cval = NULL; A->cnz = A->ccap = 0;
            return;
        }
    }
    long *cnt = (long *)calloc((size_t)m + 1, sizeof(long));
    for (long q = 0; q < nz; q++) cnt[A->crow[q] + 1]++;
    for (long r = 0; r < m; r++) cnt[r + 1] += cnt[r];
    long *pos = (long *)malloc(sizeof(long) * ((size_t)m + 1));
    memcpy(pos, cnt, sizeof(long) * ((size_t)m + 1));
    int *scol = (int *)malloc(sizeof(int) * (size_t)(nz ? nz : 1));
    double *sval = (double *)malloc(sizeof(double) * (size_t)(nz ? nz : 1));
    for (long q = 0; q < nz; q++) { long p = pos[A->crow[q]]++; scol[p] = A->ccol[q]; sval[p] = A->cval[q]; }
    A->rowptr = (long *)malloc(sizeof(long) * ((size_t)m + 1));
    A->col = (int *)malloc(sizeof(int) * (size_t)(nz ? nz : 1));
    A->val = (double *)malloc(sizeof(double) * (size_t)(nz ? nz : 1));
    long out = 0;
    for (long r = 0; r < m; r++) {
        A->rowptr[r] = out;
        const long a = cnt[r], b = cnt[r + 1];
        for (long q = a + 1; q < b; q++) {               /* stable insertion sort (rows are short) */
            int c = scol[q]; double v = sval[q]; long p = q - 1;
            while (p >= a && scol[p] > c) { scol[p + 1] = scol[p]; sval[p + 1] = sval[p]; p--; }
            scol[p + 1] = c; sval[p + 1] = v;
        }
        for (long q = a; q < b; q++) {
            if (out > A->rowptr[r] && A->col[out - 1] == scol[q]) A->val[out - 1] += sval[q];
            else { A->col[out] = scol[q]; A->val[out] = sval[q]; out++; }
        }
    }
    A->rowptr[m] = out; A->nz = out;
    free(cnt); free(pos); free(scol); free(sval);
    free(A->crow); free(A->ccol); free(A->cval); A->crow = A->ccol = NULL; A->cval = NULL; A->cnz = A->ccap = 0;
}

static int isqrt_exact(long v) { long r = (long)floor(sqrt((double)v) + 0.5); return (r * r == v) ? (int)r : -1; }

/* constant 5-point rows in lexicographic numbering, out-of-grid neighbours absent (src/solver.c:239-251) */
static int recognise_stencil(Mat A) {
    if (A->m != A->n) return 0;
    const int n = isqrt_exact(A->m);
    if (n < 1 || (n & 1) == 0) return 0;
    double c[5]; int have[5] = {0, 0, 0, 0, 0};
    for (long r = 0; r < A->m; r++) {
        const int i = (int)(r / n), j = (int)(r % n);
        long q = A->rowptr[r];
        const long e = A->rowptr[r + 1];
        const long want[5] = {i > 0 ? r - n : -1, j > 0 ? r - 1 : -1, r, j < n - 1 ? r + 1 : -1, i < n - 1 ? r + n : -1};
        for (int k = 0; k < 5; k++) {
            if (want[k] < 0) continue;
            if (q >= e || A->col[q] != want[k]) return 0;
            if (!have[k]) { c[k] = A->val[q]; have[k] = 1; }
            else if (A->val[q] != c[k]) return 0;
            q++;
        }
        if (q != e) return 0;
    }
    if (!have[2] || c[2] == 0.0) return 0;
    for (int k = 0; k < 5; k++) A->coef[k] = have[k] ? c[k] : 0.0;
    if (mgk_geom_init(&A->gf, 2, n, n, 1)) return 0;
    A->kind = MAT_STENCIL;
    return 1;
}
/* 5-point rows whose coefficients depend on the grid row i only: the stretched meshes (-mesh 1/2), where the
 * metrics are functions of y (src/mesh.c:45-107) and every row of a grid line gets the same OpA (src/solver.c:231-251) */
static int recognise_stencil_rowvar(Mat A) {
    if (A->m != A->n) return 0;
    const int n = isqrt_exact(A->m);
    if (n < 1 || (n & 1) == 0) return 0;
    double *ct = (double *)calloc((size_t)n * 5, sizeof(double)), *dt = (double *)calloc((size_t)n, sizeof(double));
    char *have = (char *)calloc((size_t)n * 5, 1);
    int ok = 1;
    for (long r = 0; r < A->m && ok; r++) {
        const int i = (int)(r / n), j = (int)(r % n);
        long q = A->rowptr[r];
        const long e = A->rowptr[r + 1];
        const long want[5] = {i > 0 ? r - n : -1, j > 0 ? r - 1 : -1, r, j < n - 1 ? r + 1 : -1, i < n - 1 ? r + n : -1};
        for (int k = 0; k < 5; k++) {
            if (want[k] < 0) continue;
            if (q >= e || A->col[q] != want[k]) { ok = 0; break; }
            if (!have[i * 5 + k]) { ct[i * 5 + k] = A->val[q]; have[i * 5 + k] = 1; }
            else if (A->val[q] != ct[i * 5 + k]) { ok = 0; break; }
            q++;
        }
        if (ok && q != e) ok = 0;
    }
    for (int i = 0; i < n && ok; i++) { if (!have[i * 5 + 2] || ct[i * 5 + 2] == 0.0) ok = 0; else dt[i] = 1.0 / ct[i * 5 + 2]; }
    free(have);
    if (!ok || mgk_geom_init(&A->gf, 2, n, n, 1)) { free(ct); free(dt); return 0; }
    A->h_ctab = ct; A->h_dtab = dt;
    A->kind = MAT_STENCIL_ROW;
    return 1;
}
static void mat_device_rowtabs(Mat A) {
    if (A->d_ctab && !A->dev_stale) return;
    const int n = A->gf.nx;
    void *p;
    if (!A->d_ctab) {
        DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)n * 5)); A->d_ctab = (double *)p;
        DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)n)); A->d_dtab = (double *)p;
        DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)n)); A->d_ones = (double *)p;
        double *ones = (double *)malloc(sizeof(double) * (size_t)n);
        for (int i = 0; i < n; i++) ones[i] = 1.0;
        DEV(mgk_h2d(G, A->d_ones, ones, sizeof(double) * (size_t)n));
        free(ones);
    }
    DEV(mgk_h2d(G, A->d_ctab, A->h_ctab, sizeof(double) * (size_t)n * 5));
    DEV(mgk_h2d(G, A->d_dtab, A->h_dtab, sizeof(double) * (size_t)n));
    A->dev_stale = 0;
}

/* full weighting rows [1 2 1;2 4 2;1 2 1]/16 centred on fine (2i+1,2j+1) (src/solver.c:1071-1092, matbuild.c:422-431) */
static int recognise_restrict(Mat A) {
    const int nc = isqrt_exact(A->m), nf = isqrt_exact(A->n);
    if (nc < 1 || nf != 2 * nc + 1) return 0;
    static const double w[3][3] = {{0.0625, 0.125, 0.0625}, {0.125, 0.25, 0.125}, {0.0625, 0.125, 0.0625}};
    for (long r = 0; r < A->m; r++) {
        const int i1 = (int)(r / nc), j1 = (int)(r % nc);
        long q = A->rowptr[r];
        if (A->rowptr[r + 1] - q != 9) return 0;
        for (int di = 0; di < 3; di++)
            for (int dj = 0; dj < 3; dj++, q++)
                if (A->col[q] != (long)(2 * i1 + di) * nf + 2 * j1 + dj || A->val[q] != w[di][dj]) return 0;
    }
    if (mgk_geom_init(&A->gf, 2, nf, nf, 1) || mgk_geom_init(&A->gc, 2, nc, nc, 1)) return 0;
    A->kind = MAT_RESTRICT;
    return 1;
}
/* bilinear rows: weights 1, 1/2, 1/4 over the 1/2/4 parents (src/solver.c:1131-1152, matbuild.c:398-407) */
static int recognise_prolong(Mat A) {
    const int nf = isqrt_exact(A->m), nc = isqrt_exact(A->n);
    if (nc < 1 || nf != 2 * nc + 1) return 0;
    for (long r = 0; r < A->m; r++) {
        const int i = (int)(r / nf), j = (int)(r % nf);
        const int ic0 = (i & 1) ? (i - 1) / 2 : i / 2 - 1, ic1 = (i & 1) ? ic0 : i / 2;
        const int jc0 = (j & 1) ? (j - 1) / 2 : j / 2 - 1, jc1 = (j & 1) ? jc0 : j / 2;
        long q = A->rowptr[r];
        const long e = A->rowptr[r + 1];
        for (int ic = ic0; ic <= ic1; ic++) {
            if (ic < 0 || ic >= nc) continue;
            for (int jc = jc0; jc <= jc1; jc++) {
                if (jc < 0 || jc >= nc) continue;
                const double wt = ((i & 1) ? 1.0 : 0.5) * ((j & 1) ? 1.0 : 0.5);
                if (q >= e || A->col[q] != (long)ic * nc + jc || A->val[q] != wt) return 0;
                q++;
            }
        }
        if (q != e) return 0;
    }
    if (mgk_geom_init(&A->gf, 2, nf, nf, 1) || mgk_geom_init(&A->gc, 2, nc, nc, 1)) return 0;
    A->kind = MAT_PROLONG;
    return 1;
}

/* The I-cycle's coupled level operator for G >= 2 grids in one level (src/solver.c:489-510 levelMatrixA = fillJacobians :214-251 +
 * fillRestrictionPortion :255-345 + fillProlongationPortion :347-470), uniform mesh, grids numbered one after the other
 * (-map 0/2 on one rank), n_(g+1) = (n_g - 1)/2:
 *     M(g,g) = A_g;   M(g0,g1) = R_k A_g1 for g1 < g0, k = g0 - g1, R_k the composite full weighting of 2S-1 points, S = 2^k
 *     (op->res[k-1], src/matbuild.c:355-396);   M(g1,g0)(f,c) = sum over the 5-point neighbours n of f INSIDE P_k's window of c of
 *     A_g1(f,n) P_k(n,c) for f in that window.
 * Checked entry by entry: the diagonal blocks are constant 5-point rows; an upper block has one value per window offset (an offset
 * whose weight came out 0.0 is absent everywhere -- the reference skips zero weights, :398); every row of a lower block equals the
 * composite weights times the recognised A_g1, accumulated here in the reference's order (differences of a few ulp from the
 * ADD_VALUES order are accepted: 1e-12 of the row's largest entry; a sum that cancels may be stored or not).  Then M x runs on the
 * stencil / transfer kernels (levelg_apply).  Windows wider than 63 points (k > 5) or more than MGP_MAXG grids: not recognised. */
static double *composite_weights(int k) {                  /* op->res[k-1]: (2^(k+1)-1)^2, built like GridTransferOperator */
    static const double r0[9] = {0.0625, 0.125, 0.0625, 0.125, 0.25, 0.125, 0.0625, 0.125, 0.0625};
    int nl = 3;
    double *dl = (double *)malloc(sizeof(double) * 9);
    memcpy(dl, r0, sizeof(r0));
    for (int l = 1; l < k; l++) {
        const int nu = 2 * nl + 1;
        double *du = (double *)calloc((size_t)nu * nu, sizeof(double));
        for (int il = 0; il < nl; il++)
            for (int jl = 0; jl < nl; jl++) {
                const int iu = 2 * (il + 1) - 1 - 1, ju = 2 * (jl + 1) - 1 - 1;
                for (int i0 = 0; i0 < 3; i0++)
                    for (int j0 = 0; j0 < 3; j0++) du[(iu + i0) * nu + (ju + j0)] += r0[i0 * 3 + j0] * dl[il * nl + jl];
            }
        free(dl); dl = du; nl = nu;
    }
    return dl;
}
static int check_levelop(Mat A, int ng, const int *n) {
    long off[MGP_MAXG + 1];
    off[0] = 0;
    for (int g = 0; g < ng; g++) off[g + 1] = off[g] + (long)n[g] * n[g];
    double cf[MGP_MAXG][5]; int havef[MGP_MAXG][5];
    memset(havef, 0, sizeof(havef));
    double *wt[MGP_MAXG][MGP_MAXG]; char *hw[MGP_MAXG][MGP_MAXG];       /* hw: 0 unknown, 1 value, 2 absent */
    double *rk[MGP_MAXG];
    memset(wt, 0, sizeof(wt)); memset(hw, 0, sizeof(hw)); memset(rk, 0, sizeof(rk));
    for (int k = 1; k < ng; k++) rk[k] = composite_weights(k);
    for (int g1 = 0; g1 < ng; g1++)
        for (int g0 = g1 + 1; g0 < ng; g0++) {
            const int W = 2 * (1 << (g0 - g1)) - 1;
            wt[g1][g0] = (double *)calloc((size_t)W * W, sizeof(double));
            hw[g1][g0] = (char *)calloc((size_t)W * W, 1);
        }
    const int Wmax = 2 * (1 << (ng - 1)) - 1, Pm = Wmax + 2;
    double *ex = (double *)malloc(sizeof(double) * (size_t)Pm * Pm);
    char *on = (char *)malloc((size_t)Pm * Pm);
    int ok = 1;
    /* pass 1: diagonal blocks and upper blocks of every row (they define A_g and the window weights); pass 2: lower blocks */
    for (int pass = 0; pass < 2 && ok; pass++)
        for (int g = 0; g < ng && ok; g++)
            for (long rr = 0; rr < (long)n[g] * n[g] && ok; rr++) {
                const long r = off[g] + rr;
                const int i = (int)(rr / n[g]), j = (int)(rr % n[g]);
                long q = A->rowptr[r];
                const long e = A->rowptr[r + 1];
                for (int g1 = 0; g1 < g && ok; g1++) {                 /* lower blocks: R_k A_g1 */
                    const int k = g - g1, S = 1 << k, W = 2 * S - 1, Pn = W + 2, nn = n[g1];
                    if (pass == 0) { while (q < e && A->col[q] < off[g1 + 1]) q++; continue; }
                    memset(ex, 0, sizeof(double) * (size_t)Pn * Pn); memset(on, 0, (size_t)Pn * Pn);
                    for (int wi = 0; wi < W; wi++)
                        for (int wj = 0; wj < W; wj++) {           /* window point (S i + wi, S j + wj) -> its 5-point row, :316-337 */
                            const int fi = S * i + wi, fj = S * j + wj;
                            const double w = rk[k][wi * W + wj];
                            if (fi - 1 >= 0) { ex[wi * Pn + wj + 1] += w * cf[g1][0]; on[wi * Pn + wj + 1] = 1; }
                            if (fj - 1 >= 0) { ex[(wi + 1) * Pn + wj] += w * cf[g1][1]; on[(wi + 1) * Pn + wj] = 1; }
                            ex[(wi + 1) * Pn + wj + 1] += w * cf[g1][2]; on[(wi + 1) * Pn + wj + 1] = 1;
                            if (fj + 1 < nn) { ex[(wi + 1) * Pn + wj + 2] += w * cf[g1][3]; on[(wi + 1) * Pn + wj + 2] = 1; }
                            if (fi + 1 < nn) { ex[(wi + 2) * Pn + wj + 1] += w * cf[g1][4]; on[(wi + 2) * Pn + wj + 1] = 1; }
                        }
                    double big = 0.0;
                    for (int t = 0; t < Pn * Pn; t++) if (fabs(ex[t]) > big) big = fabs(ex[t]);
                    for (int a = 0; a < Pn && ok; a++)                 /* ascending column = ascending (row, column) of the patch */
                        for (int b = 0; b < Pn; b++) {
                            if (!on[a * Pn + b]) continue;
                            const long colx = off[g1] + (long)(S * i - 1 + a) * nn + (S * j - 1 + b);
                            if (q < e && A->col[q] == colx) {
                                if (fabs(A->val[q] - ex[a * Pn + b]) > 1e-12 * big) { ok = 0; break; }
                                q++;
                            } else if (fabs(ex[a * Pn + b]) > 1e-12 * big) { ok = 0; break; }
                        }
                    if (ok && q < e && A->col[q] < off[g1 + 1]) ok = 0;      /* an entry of this block outside the patch */
                }
                if (!ok || pass == 1) continue;
                {                                                   /* diagonal block: constant 5-point rows (:239-251) */
                    const long want[5] = {i > 0 ? r - n[g] : -1, j > 0 ? r - 1 : -1, r, j < n[g] - 1 ? r + 1 : -1, i < n[g] - 1 ? r + n[g] : -1};
                    for (int k = 0; k < 5; k++) {
                        if (want[k] < 0) continue;
                        if (q >= e || A->col[q] != want[k]) { ok = 0; break; }
                        if (!havef[g][k]) { cf[g][k] = A->val[q]; havef[g][k] = 1; }
                        else if (A->val[q] != cf[g][k]) { ok = 0; break; }
                        q++;
                    }
                }
                for (int g0 = g + 1; g0 < ng && ok; g0++) {            /* upper blocks: window weights by offset */
                    const int S = 1 << (g0 - g), W = 2 * S - 1, nc = n[g0];
                    const int ni = ((i + 1) % S == 0) ? 1 : 2, ic0 = i / S - (ni - 1);
                    const int nj = ((j + 1) % S == 0) ? 1 : 2, jc0 = j / S - (nj - 1);
                    for (int ic = ic0; ic < ic0 + ni && ok; ic++) {
                        if (ic < 0 || ic >= nc) continue;
                        for (int jc = jc0; jc < jc0 + nj; jc++) {
                            if (jc < 0 || jc >= nc) continue;
                            const int d = (i - S * ic) * W + (j - S * jc);
                            const long colw = off[g0] + (long)ic * nc + jc;
                            if (q < e && A->col[q] == colw) {
                                if (hw[g][g0][d] == 2) { ok = 0; break; }
                                if (!hw[g][g0][d]) { wt[g][g0][d] = A->val[q]; hw[g][g0][d] = 1; }
                                else if (A->val[q] != wt[g][g0][d]) { ok = 0; break; }
                                q++;
                            } else {
                                if (hw[g][g0][d] == 1) { ok = 0; break; }
                                hw[g][g0][d] = 2;
                            }
                        }
                    }
                }
                if (ok && q != e) ok = 0;
            }
    for (int g = 0; g < ng && ok; g++) {
        for (int k = 0; k < 5; k++) if (!havef[g][k] && n[g] > 1) ok = 0;
        if (ok && (!havef[g][2] || cf[g][2] == 0.0)) ok = 0;
        if (ok && mgk_geom_init(&A->gg[g], 2, n[g], n[g], 1)) ok = 0;
    }
    if (ok) {
        A->ng = ng;
        long tot = 0;
        for (int g = 0; g < ng; g++) {
            A->goff[g] = tot; tot += A->gg[g].total;
            for (int k = 0; k < 5; k++) A->coefg[g][k] = havef[g][k] ? cf[g][k] : 0.0;
        }
        A->goff[ng] = tot;
        A->gf = A->gg[0];
        for (int g1 = 0; g1 < ng; g1++) for (int g0 = g1 + 1; g0 < ng; g0++) { A->h_wtab[g1][g0] = wt[g1][g0]; wt[g1][g0] = NULL; }
        A->kind = MAT_LEVELG;
    }
    for (int g1 = 0; g1 < ng; g1++) for (int g0 = g1 + 1; g0 < ng; g0++) { free(wt[g1][g0]); free(hw[g1][g0]); }
    for (int k = 1; k < ng; k++) free(rk[k]);
    free(ex); free(on);
    return ok;
}
static int recognise_levelop(Mat A) {
    if (A->m != A->n || A->m < 10) return 0;
    for (int nf = 3; (long)nf * nf < A->m; nf += 2) {         /* every chain nf, (nf-1)/2, ... of odd sizes whose squares add up to m */
        int n[MGP_MAXG];
        long sum = (long)nf * nf;
        n[0] = nf;
        for (int g = 1; g < MGP_MAXG && g <= 5; g++) {          /* windows of at most 63 points */
            if ((n[g - 1] & 1) == 0 || n[g - 1] < 3) break;
            n[g] = (n[g - 1] - 1) / 2;
            if ((n[g] & 1) == 0) break;
            sum += (long)n[g] * n[g];
            if (sum > A->m) break;
            if (sum == A->m) { if (check_levelop(A, g + 1, n)) return 1; break; }
        }
    }
    return 0;
}
/* 1/diag(M) in the layout of the operator's vectors (PCJACOBI on the coupled operator) and the window weights on the device */
static void mat_device_levelg(Mat A) {
    if (!A->dev_stale && A->d_dinv) return;
    const long dlen = A->goff[A->ng];
    if (!A->d_dinv) { void *pp; DEV(mgk_malloc(G, &pp, sizeof(double) * (size_t)dlen)); A->d_dinv = (double *)pp; A->d_dinv_len = dlen; }
    double *dinv = (double *)calloc((size_t)dlen, sizeof(double));
    if (!dinv) { fprintf(stderr, "[mgpetsc] FATAL: out of memory (diagonal of the level operator)\n"); exit(88); }
    for (int g = 0; g < A->ng; g++) {
        const mgk_geom *gg = &A->gg[g];
        for (int i = 0; i < gg->ny; i++) for (int j = 0; j < gg->nx; j++) dinv[A->goff[g] + gg->org + (long)i * gg->pitch + j] = 1.0 / A->coefg[g][2];
    }
    DEV(mgk_h2d(G, A->d_dinv, dinv, sizeof(double) * (size_t)dlen));
    free(dinv);
    for (int g1 = 0; g1 < A->ng; g1++)
        for (int g0 = g1 + 1; g0 < A->ng; g0++) {
            const int W = 2 * (1 << (g0 - g1)) - 1;
            if (!A->d_wtab[g1][g0]) { void *pp; DEV(mgk_malloc(G, &pp, sizeof(double) * (size_t)W * W)); A->d_wtab[g1][g0] = (double *)pp; }
            DEV(mgk_h2d(G, A->d_wtab[g1][g0], A->h_wtab[g1][g0], sizeof(double) * (size_t)W * W));
        }
    A->dev_stale = 0;
}

PetscErrorCode MatAssemblyEnd(Mat A, MatAssemblyType t) {
    if (t != MAT_FINAL_ASSEMBLY || A->assembled) return 0;
    mat_compress(A);
    A->assembled = 1;
    A->kind = MAT_GENERIC;
    if (!getenv("MGPETSC_NO_RECOGNITION"))
        if (!recognise_stencil(A) && !recognise_restrict(A) && !recognise_prolong(A) && !recognise_stencil_rowvar(A)) recognise_levelop(A);
    if (A->kind == MAT_GENERIC) {
        /* a matrix between n^2-sized index spaces keeps the padded grid layout for its vectors, so that it can
         * be mixed with recognised operators on the same grids (e.g. variable-coefficient A with the transfer
         * operators of the stretched-mesh runs, -mesh 1/2) */
        int nr = isqrt_exact(A->m), ncq = isqrt_exact(A->n);
        A->grow_ok = (nr >= 1 && (nr & 1)) && mgk_geom_init(&A->grow, 2, nr, nr, 1) == 0;
        A->gcol_ok = (ncq >= 1 && (ncq & 1)) && mgk_geom_init(&A->gcol, 2, ncq, ncq, 1) == 0;
    }
    A->dev_stale = 1; A->inv_stale = 1;
    return 0;
}

static void mat_device_csr(Mat A) {
    if (!A->dev_stale && A->d_rowptr) return;
    void *p;
    if (!A->d_rowptr) {
        DEV(mgk_malloc(G, &p, sizeof(long) * ((size_t)A->m + 1))); A->d_rowptr = (long *)p;
        DEV(mgk_malloc(G, &p, sizeof(int) * (size_t)(A->nz ? A->nz : 1))); A->d_col = (int *)p;
        DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)(A->nz ? A->nz : 1))); A->d_val = (double *)p;
        DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)(A->m ? A->m : 1))); A->d_dinv = (double *)p;
    }
    DEV(mgk_h2d(G, A->d_rowptr, A->rowptr, sizeof(long) * ((size_t)A->m + 1)));
    if (A->gcol_ok) {                                    /* columns -> offsets into the padded x field */
        int *pc = (int *)malloc(sizeof(int) * (size_t)(A->nz ? A->nz : 1));
        const int n = A->gcol.nx;
        for (long q = 0; q < A->nz; q++) pc[q] = (int)(A->gcol.org + (long)(A->col[q] / n) * A->gcol.pitch + A->col[q] % n);
        DEV(mgk_h2d(G, A->d_col, pc, sizeof(int) * (size_t)A->nz));
        free(pc);
    } else {
        DEV(mgk_h2d(G, A->d_col, A->col, sizeof(int) * (size_t)A->nz));
    }
    DEV(mgk_h2d(G, A->d_val, A->val, sizeof(double) * (size_t)A->nz));
    /* PCJACOBI: 1/diag in the layout of the row vectors */
    /* (length = nalloc of a row vector, see vec_new: the flat BLAS-1 kernels run over whole allocations; sized A->m the
     *  pointwise multiply of KSPSolve read up to 15 doubles past the end -- found by the sanitized CPU build) */
    long dlen = A->grow_ok ? A->grow.total : ((long)A->m + 15) / 16 * 16;
    if (dlen < 16) dlen = 16;
    if (!A->d_dinv_len) { void *pp; DEV(mgk_malloc(G, &pp, sizeof(double) * (size_t)(dlen ? dlen : 1))); mgk_free(G, A->d_dinv); A->d_dinv = (double *)pp; A->d_dinv_len = dlen; }
    double *dinv = (double *)calloc((size_t)(dlen ? dlen : 1), sizeof(double));
    for (long r = 0; r < A->m; r++) {
        double d = 0.0;
        for (long q = A->rowptr[r]; q < A->rowptr[r + 1]; q++) if (A->col[q] == r) d = A->val[q];
        const long o = A->grow_ok ? A->grow.org + (r / A->grow.nx) * A->grow.pitch + r % A->grow.nx : r;
        dinv[o] = 1.0 / d;
    }
    DEV(mgk_h2d(G, A->d_dinv, dinv, sizeof(double) * (size_t)dlen));
    free(dinv);
    A->dev_stale = 0;
}

PetscErrorCode MatCreateVecs(Mat A, Vec *right, Vec *left) {       /* src/solver.c:1172: (u, b) */
    const mgk_geom *gr = NULL, *gl = NULL;
    if (A->kind == MAT_STENCIL || A->kind == MAT_STENCIL_ROW) gr = gl = &A->gf;
    else if (A->kind == MAT_RESTRICT) { gr = &A->gf; gl = &A->gc; }
    else if (A->kind == MAT_PROLONG) { gr = &A->gc; gl = &A->gf; }
    else if (A->kind == MAT_LEVELG) {
        if (right) *right = vec_newg(A->ng, A->gg);
        if (left) *left = vec_newg(A->ng, A->gg);
        return 0;
    }
    else { if (A->gcol_ok) gr = &A->gcol; if (A->grow_ok) gl = &A->grow; }
    if (right) *right = vec_new(A->n, gr);
    if (left) *left = vec_new(A->m, gl);
    return 0;
}
PetscErrorCode MatGetSize(Mat A, PetscInt *m, PetscInt *n) { if (m) *m = A->m; if (n) *n = A->n; return 0; }

static int geom_eq(const mgk_geom *a, const mgk_geom *b) { return a->dim == b->dim && a->nx == b->nx && a->ny == b->ny && a->nz == b->nz; }
static void need_vec(Vec v, int padded, const mgk_geom *g, PetscInt n, const char *who) {
    int ok = (v->n == n) && (v->padded == padded) && (!padded || geom_eq(&v->g, g));
    if (!ok) { fprintf(stderr, "[mgpetsc] FATAL: %s: vector does not match the operator's layout (create it with MatCreateVecs/VecDuplicate)\n", who); exit(88); }
}

/* y = A x (addto == NULL) or y = addto + alpha*(A x) on the assembled AIJ operator; vectors in the operator's layouts */
static void csr_apply(Mat A, Vec x, Vec y, double alpha, Vec addto, const char *who) {
    need_vec(x, A->gcol_ok, &A->gcol, A->n, who);
    need_vec(y, A->grow_ok, &A->grow, A->m, who);
    if (addto) need_vec(addto, A->grow_ok, &A->grow, A->m, who);
    mat_device_csr(A);
    (void)vdev(x); if (addto) (void)vdev(addto);
    lz_before_write(y, addto != y);
    y->host_dirty = 0;
    DEV(mgk_csr_mult_f64(G, A->m, A->d_rowptr, A->d_col, A->d_val, vdev(x), y->dev, alpha, addto ? vdev(addto) : NULL,
                         A->grow_ok ? A->grow.nx : 0, A->grow_ok ? A->grow.pitch : 0, A->grow_ok ? A->grow.org : 0, NULL));
}

/* the same on the recognised level operator of several grids: with s_0 = A_0 x_0, s_g = R s_(g-1) + A_g x_g the lower triangle and
 * the diagonal are one cascade down the grids; then every upper block adds its window sums.  Vectors in the composite layout */
static Vec mat_work(Mat A, Vec like);
static void rr_now(Mat Af, Mat Rm, Vec bf, Vec uf, Vec bc, double *uc0, double dinv_c, double scale_c, const double *dtab_c);
static void need_vecg(Mat A, Vec v, const char *who) {
    if (!(v->padded == 2 && v->ng == A->ng && geom_eq(&v->gg[0], &A->gg[0]))) {
        fprintf(stderr, "[mgpetsc] FATAL: %s: vector does not match the operator's layout (create it with MatCreateVecs/VecDuplicate)\n", who); exit(88);
    }
}
static void levelg_apply(Mat A, Vec x, Vec y, double alpha, Vec addto, const char *who) {
    need_vecg(A, x, who); need_vecg(A, y, who);
    if (addto) need_vecg(A, addto, who);
    if (x == y) UNSUPPORTED("the level operator applied in place");
    mat_device_levelg(A);
    const double *xd = vdev(x), *ad = addto ? vdev(addto) : NULL;
    lz_before_write(y, addto != y);
    Vec t = (addto || alpha != 1.0) ? mat_work(A, y) : y;    /* M x first, then the combination (x may be read until the end) */
    if (t == x) UNSUPPORTED("the level operator applied onto its own work vector");
    for (int g = 0; g < A->ng; g++) {
        if (g == 0) DEV(mgk_apply_f64(G, &A->gg[0], A->coefg[0], xd, t->dev, NULL));
        else {
            DEV(mgk_restrict_fw_f64(G, &A->gg[g - 1], &A->gg[g], t->dev + A->goff[g - 1], t->dev + A->goff[g], NULL));
            DEV(mgk_apply_add_f64(G, &A->gg[g], A->coefg[g], xd + A->goff[g], t->dev + A->goff[g], NULL));
        }
    }
    for (int g1 = 0; g1 < A->ng; g1++)
        for (int g0 = g1 + 1; g0 < A->ng; g0++)
            DEV(mgk_window_add_f64(G, &A->gg[g1], &A->gg[g0], 1 << (g0 - g1), A->d_wtab[g1][g0], xd + A->goff[g0], t->dev + A->goff[g1], NULL));
    t->host_dirty = 0;
    y->host_dirty = 0;
    if (t != y) {
        if (ad) {                                                                            /* y = addto + alpha t */
            if (y->dev != ad) DEV(mgk_d2d(G, y->dev, ad, sizeof(double) * (size_t)y->nalloc, NULL));
            DEV(mgk_flat_axpy(G, y->nalloc, alpha, t->dev, y->dev, NULL));
        } else { DEV(mgk_d2d(G, y->dev, t->dev, sizeof(double) * (size_t)y->nalloc, NULL)); DEV(mgk_flat_scale(G, y->nalloc, alpha, y->dev, NULL)); }
    }
}

PetscErrorCode MatMult(Mat A, Vec x, Vec y) {                       /* src/solver.c:1516,1535,1540 */
    if (!A->assembled) UNSUPPORTED("MatMult on an unassembled matrix");
    if (x == y) UNSUPPORTED("MatMult with x == y");
    if (tc_mult(A, x, y)) return 0;
    if (A->kind == MAT_RESTRICT && x->lz == LZ_RESIDUAL && x->lz_A->gf.dim == 2 && geom_eq(&x->lz_A->gf, &A->gf) && y->padded == 1 && geom_eq(&y->g, &A->gc) &&
        y != x->lz_b && y != x->lz_x) {
        /* b_c = R (b - A u) with the residual not computed yet (src/solver.c:1534-1535): one pass, r stays deferred */
        /* ... and b_c is deferred in turn: the coarse KSPSolve from the zero guess takes its first sweep out of the same pass */
        struct _p_Mat *Af = x->lz_A;
        Vec bf = x->lz_b, uf = x->lz_x;
        (void)vdev(bf); (void)vdev(uf);
        lz_before_write(y, 1);
        y->host_dirty = 0;
        if (lazy_on() == 2) { rr_now(Af, A, bf, uf, y, NULL, 1.0, 1.0, NULL); return 0; }
        lz_register(y, LZ_RR, Af, bf, uf);
        y->lz_A2 = A;
        return 0;
    }
    if (A->kind == MAT_PROLONG && lazy_on() && x->padded == 1 && y->padded == 1 && geom_eq(&x->g, &A->gc) && geom_eq(&y->g, &A->gf)) {
        (void)vdev(x);                                       /* rv = P u_c: deferred (src/solver.c:1540) */
        lz_before_write(y, 1);
        y->host_dirty = 0;
        lz_register(y, LZ_PROLONG, A, NULL, x);
        return 0;
    }
    (void)vdev(x);
    if (A->kind != MAT_GENERIC && A->kind != MAT_LEVELG) lz_before_write(y, 1);
    y->host_dirty = 0;
    switch (A->kind) {
    case MAT_STENCIL:
        need_vec(x, 1, &A->gf, A->n, "MatMult"); need_vec(y, 1, &A->gf, A->m, "MatMult");
        DEV(mgk_apply_f64(G, &A->gf, A->coef, vdev(x), y->dev, NULL));
        break;
    case MAT_STENCIL_ROW:
        need_vec(x, 1, &A->gf, A->n, "MatMult"); need_vec(y, 1, &A->gf, A->m, "MatMult");
        mat_device_rowtabs(A);
        DEV(mgk_rowcoef_f64(G, &A->gf, 4, A->d_ctab, A->d_dtab, 1.0, NULL, vdev(x), y->dev, NULL));
        break;
    case MAT_RESTRICT:
        need_vec(x, 1, &A->gf, A->n, "MatMult"); need_vec(y, 1, &A->gc, A->m, "MatMult");
        DEV(mgk_restrict_fw_f64(G, &A->gf, &A->gc, vdev(x), y->dev, NULL));
        break;
    case MAT_PROLONG:
        need_vec(x, 1, &A->gc, A->n, "MatMult"); need_vec(y, 1, &A->gf, A->m, "MatMult");
        DEV(mgk_memset0(G, y->dev, sizeof(double) * (size_t)y->nalloc, NULL));      /* y = 0 + P x */
        DEV(mgk_prolong_add_f64(G, &A->gf, &A->gc, vdev(x), y->dev, NULL));
        break;
    case MAT_LEVELG:
        levelg_apply(A, x, y, 1.0, NULL, "MatMult");
        break;
    default:
        csr_apply(A, x, y, 1.0, NULL, "MatMult");
    }
    return 0;
}
static Vec mat_work(Mat A, Vec like) { if (!A->work) VecDuplicate(like, &A->work); return A->work; }
PetscErrorCode MatMultAdd(Mat A, Vec x, Vec y, Vec z) {            /* z = y + A x */
    if (A->kind == MAT_GENERIC) { csr_apply(A, x, z, 1.0, y, "MatMultAdd"); return 0; }
    if (A->kind == MAT_LEVELG) { levelg_apply(A, x, z, 1.0, y, "MatMultAdd"); return 0; }
    if (A->kind == MAT_PROLONG && z == y) {                       /* u_f += P u_c in one pass (MatInterpolateAdd) */
        need_vec(x, 1, &A->gc, A->n, "MatMultAdd"); need_vec(y, 1, &A->gf, A->m, "MatMultAdd");
        (void)vdev(x); (void)vdev(y);
        lz_before_write(y, 0);
        if (lazy_on() && x != y) { lz_register(y, LZ_ADDP, A, NULL, x); return 0; }      /* the smoother that follows fuses it (PCMG) */
        DEV(mgk_prolong_add_f64(G, &A->gf, &A->gc, vdev(x), vdev(y), NULL));
        return 0;
    }
    Vec t = mat_work(A, y);
    MatMult(A, x, t);
    (void)vdev(t);                                          /* the work vector is not a deferred temporary */
    if (z != y) VecCopy(y, z);
    return VecAXPY(z, 1.0, t);
}
static void mat_residual_now(Mat A, Vec b, Vec x, Vec r);
PetscErrorCode MatResidual(Mat A, Vec b, Vec x, Vec r) {           /* r = b - A x */
    if (tc_resid(A, b, x, r)) return 0;
    if ((A->kind == MAT_STENCIL || A->kind == MAT_STENCIL_ROW) && lazy_on() && r != b && r != x && r->padded == 1 && geom_eq(&r->g, &A->gf)) {
        need_vec(x, 1, &A->gf, A->n, "MatResidual"); need_vec(b, 1, &A->gf, A->m, "MatResidual");
        (void)vdev(b); (void)vdev(x);                        /* operands concrete */
        lz_before_write(r, 1);
        r->host_dirty = 0;
        lz_register(r, LZ_RESIDUAL, A, b, x);                /* deferred: the restriction that follows forms it on the fly */
        return 0;
    }
    mat_residual_now(A, b, x, r);
    return 0;
}
/* b_c = R (b - A u) in one pass, optionally with the coarse level's first sweep from its zero guess (uc0 = scale_c * (b_c * dinv_c)) */
static void rr_now(Mat Af, Mat Rm, Vec bf, Vec uf, Vec bc, double *uc0, double dinv_c, double scale_c, const double *dtab_c) {
    const double *bd = vdev(bf), *ud = vdev(uf);
    g_lzstat[0]++;
    if (Af->kind == MAT_STENCIL) DEV(mgk_residual_restrict_2d_f64(G, &Rm->gf, &Rm->gc, Af->coef, bd, ud, bc->dev, uc0, dinv_c, scale_c, NULL));
    else { mat_device_rowtabs(Af); DEV(mgk_residual_restrict_2d_rowcoef_f64(G, &Rm->gf, &Rm->gc, Af->d_ctab, bd, ud, bc->dev, uc0, dtab_c, scale_c, NULL)); }
}
/* a deferred value is needed after all */
static void lz_settle(Vec v) {
    const int kind = v->lz;
    struct _p_Mat *A = v->lz_A; Vec b = v->lz_b, x = v->lz_x;
    struct _p_Mat *A2 = v->lz_A2;
    if (!kind) return;
    if (kind == LZ_TAIL) {
        /* a recording that is replayed call by call goes through the ordinary paths, which defer in their turn: the restricted right-hand
         * side it had taken comes back as LZ_RR.  The caller wants the value, so that is computed too (a Chebyshev KSPSolve on it -- which
         * the recorder is not asked about -- read the buffer before the restriction had run) */
        tc_settle(v);
        if (v->lz && v->lz != LZ_TAIL) lz_settle(v);
        return;
    }
    lz_drop(v);
    if (kind == LZ_RR) { rr_now(A, A2, b, x, v, NULL, 1.0, 1.0, NULL); return; }
    g_lzstat[1 + kind]++;
    if (kind == LZ_RESIDUAL) mat_residual_now(A, b, x, v);
    else if (kind == LZ_PROLONG) {
        DEV(mgk_memset0(G, v->dev, sizeof(double) * (size_t)v->nalloc, NULL));      /* v = 0 + P x */
        DEV(mgk_prolong_add_f64(G, &A->gf, &A->gc, vdev(x), v->dev, NULL));
    } else if (kind == LZ_ADDP) DEV(mgk_prolong_add_f64(G, &A->gf, &A->gc, vdev(x), v->dev, NULL));
}
static void mat_residual_now(Mat A, Vec b, Vec x, Vec r) {
    (void)vdev(b); (void)vdev(x);
    lz_before_write(r, r != b && r != x);
    r->host_dirty = 0;
    if (A->kind == MAT_STENCIL) {
        need_vec(x, 1, &A->gf, A->n, "MatResidual");
        DEV(mgk_residual_f64(G, &A->gf, A->coef, vdev(b), vdev(x), r->dev, NULL));
        return;
    }
    if (A->kind == MAT_STENCIL_ROW) {
        need_vec(x, 1, &A->gf, A->n, "MatResidual");
        mat_device_rowtabs(A);
        DEV(mgk_rowcoef_f64(G, &A->gf, 1, A->d_ctab, A->d_dtab, 1.0, vdev(b), vdev(x), r->dev, NULL));
        return;
    }
    if (A->kind == MAT_GENERIC) { csr_apply(A, x, r, -1.0, b, "MatResidual"); return; }
    if (A->kind == MAT_LEVELG) { levelg_apply(A, x, r, -1.0, b, "MatResidual"); return; }
    MatMult(A, x, r);
    VecAYPX(r, -1.0, b);
}
PetscErrorCode MatScale(Mat A, PetscScalar a) {
    lz_before_mat_change(A);
    for (long q = 0; q < A->nz; q++) A->val[q] *= a;
    for (int k = 0; k < 7; k++) A->coef[k] *= a;
    for (int g = 0; g < A->ng; g++) {
        for (int k = 0; k < 5; k++) A->coefg[g][k] *= a;
        for (int g0 = g + 1; g0 < A->ng; g0++) { const int W = 2 * (1 << (g0 - g)) - 1; for (int k = 0; k < W * W; k++) A->h_wtab[g][g0][k] *= a; }
    }
    if (A->kind == MAT_RESTRICT || A->kind == MAT_PROLONG) A->kind = MAT_GENERIC;     /* weights no longer the canonical ones */
    if (A->kind == MAT_STENCIL_ROW) {
        const int n = A->gf.nx;
        for (int i = 0; i < n * 5; i++) A->h_ctab[i] *= a;
        for (int i = 0; i < n; i++) A->h_dtab[i] = 1.0 / A->h_ctab[i * 5 + 2];
    }
    A->dev_stale = 1; A->inv_stale = 1;
    return 0;
}
PetscErrorCode MatMatMult(Mat A, Mat B, MatReuse s, PetscReal f, Mat *C) { (void)A; (void)B; (void)s; (void)f; (void)C; UNSUPPORTED("MatMatMult (additive cycles)"); return 1; }
PetscErrorCode MatView(Mat A, PetscViewer v) {
    (void)v;
    static const char *kinds[] = {"assembled AIJ (generic CSR kernel)", "matrix-free 5-point stencil", "matrix-free full weighting", "matrix-free bilinear prolongation",
                                  "matrix-free 5-point stencil with row-dependent coefficients",
                                  "matrix-free level operator of several grids [A_g on the diagonal, R^k A_g below, A_g P^k | window above] (stencil + transfer kernels)"};
    printf("Mat Object: %d x %d, %ld nonzeros, device operator: %s\n", A->m, A->n, A->nz, kinds[A->kind]);
    fflush(stdout);
    return 0;
}
PetscErrorCode MatDestroy(Mat *pA) {
    if (!pA || !*pA) return 0;
    Mat A = *pA;
    lz_before_mat_change(A);
    free(A->crow); free(A->ccol); free(A->cval); free(A->rowptr); free(A->col); free(A->val);
    if (G) {
        if (A->d_rowptr) mgk_free(G, A->d_rowptr);
        if (A->d_col) mgk_free(G, A->d_col);
        if (A->d_val) mgk_free(G, A->d_val);
        if (A->d_dinv) mgk_free(G, A->d_dinv);
        if (A->d_ctab) mgk_free(G, A->d_ctab);
        if (A->d_dtab) mgk_free(G, A->d_dtab);
        if (A->d_ones) mgk_free(G, A->d_ones);
        if (A->d_inv) mgk_free(G, A->d_inv);
        if (A->d_c1) mgk_free(G, A->d_c1);
        if (A->d_c2) mgk_free(G, A->d_c2);
        for (int a = 0; a < MGP_MAXG; a++) for (int b = 0; b < MGP_MAXG; b++) if (A->d_wtab[a][b]) mgk_free(G, A->d_wtab[a][b]);
    }
    for (int a = 0; a < MGP_MAXG; a++) for (int b = 0; b < MGP_MAXG; b++) free(A->h_wtab[a][b]);
    if (A->work) VecDestroy(&A->work);
    free(A->h_ctab); free(A->h_dtab);
    free(A); *pA = NULL;
    return 0;
}

/* ------------------------------------------------------------------ */
/* KSP / PC                                                            */
/* ------------------------------------------------------------------ */
enum { K_RICHARDSON = 0, K_CHEBYSHEV = 1, K_OTHER = 2, K_PREONLY = 3 };
enum { P_DEFAULT = 0, P_JACOBI = 1, P_NONE = 2, P_MG = 3, P_LU = 4 };
/* PCMG state (-cycle 8, src/solver.c:1918-1956).  PETSc numbers levels coarse-to-fine: 0 = coarsest. */
typedef struct pcmg {
    int levels;
    KSP *smooth;                /* [0] coarse solve, [i>0] level smoother (used down and up) */
    Mat *interp, *restr;        /* [i] between level i-1 and i */
    Vec *b, *x, *r;             /* user-provided work vectors (PCMGSetRhs/X/R) or created on demand */
    unsigned char *own_b, *own_x, *own_r;
} pcmg;
struct _p_PC { KSP ksp; pcmg *mg; };
struct _p_KSP {
    Mat A;
    int type, pc;
    double scale, emin, emax;
    PetscInt maxits;
    int guess_nonzero;
    KSPNormType normtype;
    Vec work[3];
    Vec b, x;                   /* vec_rhs / vec_sol of the last KSPSolve (KSPBuildResidual, src/solver.c:1534) */
    PetscInt its;
    char prefix[64];
    double rtol, atol, dtol;    /* used only by the outer Richardson of -cycle 8 (norm type != NONE) */
    PetscReal *hist; PetscInt nhist;
    int type_from_user;
    int spec_ok; Vec spec_b, spec_x; unsigned long spec_vb, spec_vx, spec_epoch;   /* work[0] holds J(spec_x) made by the norm pass (below) */
    int spec_n;                 /* ... how many sweeps that pass made: 1, or 3 (2-D, round 3: mgk_jacobi3_2d_sumsq_store_f64) */
    struct _p_PC pcobj;
};

PetscErrorCode KSPCreate(MPI_Comm comm, KSP *out) {
    (void)comm;
    need_ctx();
    KSP k = (KSP)calloc(1, sizeof(*k));
    k->type = K_OTHER;          /* PETSc's default is GMRES: a type must be chosen */
    k->pc = P_DEFAULT; k->scale = 1.0; k->maxits = 10000; k->normtype = KSP_NORM_DEFAULT;
    k->rtol = 1.e-5; k->atol = 1.e-50; k->dtol = 1.e5;
    k->pcobj.ksp = k;
    *out = k;
    return 0;
}
static int ksp_type_from(const char *t) {
    if (!strcmp(t, KSPRICHARDSON)) return K_RICHARDSON;
    if (!strcmp(t, KSPCHEBYSHEV)) return K_CHEBYSHEV;
    if (!strcmp(t, KSPPREONLY)) return K_PREONLY;
    return K_OTHER;
}
static int pc_type_from(const char *t) {
    if (!strcmp(t, PCJACOBI)) return P_JACOBI;
    if (!strcmp(t, PCNONE)) return P_NONE;
    if (!strcmp(t, PCLU) || !strcmp(t, "cholesky")) return P_LU;      /* exact solve on a small grid (PCMG's coarse solver) */
    fprintf(stderr, "[mgpetsc] FATAL: -pc_type %s is not provided by this drop-in (available: jacobi, none, lu on <= 1024 unknowns)\n", t);
    exit(87);
}
/* (every setter that changes what a sweep IS drops the speculative first sweep the last norm pass may have left in work[0]: it was made
 * with the old scale / preconditioner / type -- ADVICE round 2) */
PetscErrorCode KSPSetType(KSP k, KSPType t) { k->type = ksp_type_from(t); k->type_from_user = 1; k->spec_ok = 0; return 0; }
/* (the sweep's work vector is created here, not inside the first KSPSolve: a 134 MB hipMalloc takes ~2 ms, a third of the reference's whole
 * `Solver walltime` at 4097^2 -- PETSc creates its work vectors in KSPSetUp, which the reference never calls explicitly; ksp_work replaces it
 * if a solve comes with another layout) */
PetscErrorCode KSPSetOperators(KSP k, Mat A, Mat P) {
    (void)P; k->A = A; k->spec_ok = 0;
    if (A && A->assembled && (A->kind == MAT_STENCIL || A->kind == MAT_STENCIL_ROW) && !k->work[0]) MatCreateVecs(A, &k->work[0], NULL);
    return 0;
}
PetscErrorCode KSPSetNormType(KSP k, KSPNormType n) { k->normtype = n; k->spec_ok = 0; return 0; }
PetscErrorCode KSPSetTolerances(KSP k, PetscReal rtol, PetscReal atol, PetscReal dtol, PetscInt maxits) {
    /* KSP_NORM_NONE (the smoothers): only max_it matters (src/solver.c:1473-1474); the tolerances are kept for the
     * outer Richardson of -cycle 8 (src/solver.c:1924) */
    if (rtol != PETSC_DEFAULT) k->rtol = rtol;
    if (atol != PETSC_DEFAULT) k->atol = atol;
    if (dtol != PETSC_DEFAULT) k->dtol = dtol;
    if (maxits != PETSC_DEFAULT) k->maxits = maxits;
    return 0;
}
PetscErrorCode KSPRichardsonSetScale(KSP k, PetscReal s) { k->scale = s; k->spec_ok = 0; return 0; }
PetscErrorCode KSPChebyshevSetEigenvalues(KSP k, PetscReal emax, PetscReal emin) { k->emax = emax; k->emin = emin; k->spec_ok = 0; return 0; }
PetscErrorCode PetscObjectSetOptionsPrefix(void *obj, const char prefix[]) {
    KSP k = (KSP)obj;           /* the reference only prefixes KSPs (src/solver.c:1624,1634,1643) */
    snprintf(k->prefix, sizeof(k->prefix), "%s", prefix ? prefix : "");
    return 0;
}
static const char *kopt(KSP k, const char *name) {
    char key[128];
    snprintf(key, sizeof(key), "-%s%s", k->prefix, name);
    return opt_get(key);
}
PetscErrorCode KSPSetFromOptions(KSP k) {                         /* src/solver.c:1476,1492,1509 */
    const char *v;
    k->spec_ok = 0;
    if ((v = kopt(k, "ksp_type")) && v[0]) { k->type = ksp_type_from(v); k->type_from_user = 1; }
    if ((v = kopt(k, "pc_type")) && v[0]) k->pc = pc_type_from(v);
    if ((v = kopt(k, "ksp_richardson_scale")) && v[0]) k->scale = strtod(v, NULL);
    if ((v = kopt(k, "ksp_max_it")) && v[0]) k->maxits = (PetscInt)strtol(v, NULL, 10);
    if ((v = kopt(k, "ksp_chebyshev_eigenvalues")) && v[0]) {
        char *end;
        k->emin = strtod(v, &end);
        while (*end == ',' || *end == ' ') end++;
        k->emax = strtod(end, NULL);
    }
    if (k->pc == P_MG && k->pcobj.mg)            /* PCSetFromOptions_MG: the level solvers read -mg_coarse_* / -mg_levels_* */
        for (int i = 0; i < k->pcobj.mg->levels; i++) KSPSetFromOptions(k->pcobj.mg->smooth[i]);
    return 0;
}
PetscErrorCode KSPSetInitialGuessNonzero(KSP k, PetscBool f) { k->guess_nonzero = (f == PETSC_TRUE); k->spec_ok = 0; return 0; }
PetscErrorCode KSPGetPC(KSP k, PC *pc) { *pc = &k->pcobj; return 0; }
PetscErrorCode PCSetType(PC pc, PCType t) {
    pc->ksp->spec_ok = 0;
    if (!strcmp(t, PCMG)) { pc->ksp->pc = P_MG; return 0; }
    pc->ksp->pc = pc_type_from(t);
    return 0;
}
PetscErrorCode KSPGetIterationNumber(KSP k, PetscInt *its) { *its = k->its; return 0; }
PetscErrorCode KSPSetResidualHistory(KSP k, PetscReal a[], PetscInt na, PetscBool r) {      /* src/solver.c:1923 */
    (void)r; k->hist = a; k->nhist = na; return 0;
}
PetscErrorCode KSPMonitorSet(KSP k, PetscErrorCode (*m)(KSP, PetscInt, PetscReal, void *), void *c, PetscErrorCode (*d)(void **)) {
    (void)k; (void)m; (void)c; (void)d; UNSUPPORTED("KSPMonitorSet (delayed cycles)"); return 1;
}

/* ---- PCMG (-cycle 8, MultigridPetscPCMG, src/solver.c:1884-1989) ----
 * Multiplicative V-cycle, one cycle per application, the textbook PCMG recursion:
 *   x_L = 0;  level i > 0:  smooth(b_i, x_i);  r_i = b_i - A_i x_i;  b_{i-1} = R_i r_i;  x_{i-1} = 0;  recurse;
 *                           x_i += P_i x_{i-1};  smooth(b_i, x_i);       level 0:  coarse solve(b_0, x_0)
 * Level solvers are ordinary KSPs of this shim (richardson / chebyshev / preonly + jacobi / none / lu, KSP_NORM_NONE, max_it
 * sweeps) configured through -mg_levels_* and -mg_coarse_*.  The COARSE solve defaults to PETSc's own default, preonly + LU: an
 * exact solve with the dense inverse of the coarsest operator (mg_setup, ksp_solve_direct; <= 1024 unknowns).  PETSc's default
 * LEVEL smoother (chebyshev + SOR with eigenvalues estimated by GMRES) is not provided: without -mg_levels_* options the level
 * solvers fall back, with a note, to richardson + jacobi, 2 sweeps.  The PETSc version is unpinned and PCMG's internals are
 * version dependent: parity of this path is pinned only against the oracle's restatement of the recursion above (oracle/mgo.c,
 * mgo_pcmg) and a dense numpy restatement with an exact coarse solve (tests/test_petsc_shim_gpu.py). */
static pcmg *need_mg(PC pc, const char *who) {
    if (pc->ksp->pc != P_MG || !pc->mg) { fprintf(stderr, "[mgpetsc] FATAL: %s before PCSetType(PCMG) + PCMGSetLevels\n", who); exit(86); }
    return pc->mg;
}
static int mg_level(pcmg *mg, PetscInt l, const char *who) {
    if (l < 0 || l >= mg->levels) { fprintf(stderr, "[mgpetsc] FATAL: %s: level %d outside 0..%d\n", who, (int)l, mg->levels - 1); exit(86); }
    return (int)l;
}
PetscErrorCode PCMGSetLevels(PC pc, PetscInt l, MPI_Comm *c) {
    (void)c;
    if (pc->ksp->pc != P_MG) UNSUPPORTED("PCMGSetLevels on a PC that is not PCMG");
    if (pc->mg) UNSUPPORTED("PCMGSetLevels called twice");
    if (l < 1) UNSUPPORTED("PCMGSetLevels with fewer than one level");
    pcmg *mg = (pcmg *)calloc(1, sizeof(pcmg));
    mg->levels = (int)l;
    mg->smooth = (KSP *)calloc((size_t)l, sizeof(KSP));
    mg->interp = (Mat *)calloc((size_t)l, sizeof(Mat)); mg->restr = (Mat *)calloc((size_t)l, sizeof(Mat));
    mg->b = (Vec *)calloc((size_t)l, sizeof(Vec)); mg->x = (Vec *)calloc((size_t)l, sizeof(Vec)); mg->r = (Vec *)calloc((size_t)l, sizeof(Vec));
    mg->own_b = (unsigned char *)calloc((size_t)l, 1); mg->own_x = (unsigned char *)calloc((size_t)l, 1); mg->own_r = (unsigned char *)calloc((size_t)l, 1);
    for (int i = 0; i < mg->levels; i++) {
        KSPCreate(PETSC_COMM_WORLD, &mg->smooth[i]);
        PetscObjectSetOptionsPrefix(mg->smooth[i], i == 0 ? "mg_coarse_" : "mg_levels_");
        mg->smooth[i]->normtype = KSP_NORM_NONE;
        mg->smooth[i]->maxits = 2;                        /* PETSc's default number of smoothing steps */
        mg->smooth[i]->guess_nonzero = (i > 0);           /* x is zeroed explicitly by the cycle */
    }
    pc->mg = mg;
    return 0;
}
PetscErrorCode PCMGGetCoarseSolve(PC pc, KSP *k) { *k = need_mg(pc, "PCMGGetCoarseSolve")->smooth[0]; return 0; }
PetscErrorCode PCMGGetSmoother(PC pc, PetscInt l, KSP *k) { pcmg *mg = need_mg(pc, "PCMGGetSmoother"); *k = mg->smooth[mg_level(mg, l, "PCMGGetSmoother")]; return 0; }
PetscErrorCode PCMGSetInterpolation(PC pc, PetscInt l, Mat m) { pcmg *mg = need_mg(pc, "PCMGSetInterpolation"); mg->interp[mg_level(mg, l, "PCMGSetInterpolation")] = m; return 0; }
PetscErrorCode PCMGSetRestriction(PC pc, PetscInt l, Mat m) { pcmg *mg = need_mg(pc, "PCMGSetRestriction"); mg->restr[mg_level(mg, l, "PCMGSetRestriction")] = m; return 0; }
PetscErrorCode PCMGSetR(PC pc, PetscInt l, Vec c) { pcmg *mg = need_mg(pc, "PCMGSetR"); mg->r[mg_level(mg, l, "PCMGSetR")] = c; return 0; }
PetscErrorCode PCMGSetRhs(PC pc, PetscInt l, Vec c) { pcmg *mg = need_mg(pc, "PCMGSetRhs"); mg->b[mg_level(mg, l, "PCMGSetRhs")] = c; return 0; }
PetscErrorCode PCMGSetX(PC pc, PetscInt l, Vec c) { pcmg *mg = need_mg(pc, "PCMGSetX"); mg->x[mg_level(mg, l, "PCMGSetX")] = c; return 0; }

/* No -pc_type: PETSc would use ILU(0) (block Jacobi + ILU(0) on several ranks), which this drop-in does not provide.
 * MGPETSC_DEFAULT_PC=jacobi opts in to the substitution silently; MGPETSC_DEFAULT_PC=refuse makes the run stop instead of
 * producing numbers that differ from a PETSc run while looking like one; otherwise Jacobi is substituted and the run says so
 * on stderr AND in its stdout report (and in KSPView), once. */
static int ksp_pc(KSP k) {
    if (k->pc == P_DEFAULT) {
        if (!g_notice_pc) {
            const char *e = getenv("MGPETSC_DEFAULT_PC");
            if (e && !strcmp(e, "refuse")) {
                fprintf(stderr, "[mgpetsc] no -pc_type given: PETSc's default preconditioner (ILU(0)) is not provided and "
                                "MGPETSC_DEFAULT_PC=refuse is set; pass -pc_type jacobi\n");
                exit(2);
            }
            if (!(e && !strcmp(e, "jacobi"))) {
                fprintf(stderr, "[mgpetsc] note: PETSc's default preconditioner (ILU(0)) is not provided; "
                                "using -pc_type jacobi (pass it explicitly to silence this note)\n");
                printf("[mgpetsc] -pc_type not given: Jacobi substituted for PETSc's default ILU(0); iteration counts differ from a PETSc run\n");
            }
            g_notice_pc = 1;
        }
        return P_JACOBI;
    }
    return k->pc;
}
/* work vector q of solver k, about to be WRITTEN: a deferred residual may name it as its iterate (KSPSolve moves the dependency of a
 * residual whose norm pass left it deferred from x to the work vector that receives x's old buffer, see there) and is computed first */
static Vec ksp_work(KSP k, int q, Vec like) {
    if (k->work[q] && !same_layout(k->work[q], like)) VecDestroy(&k->work[q]);
    if (!k->work[q]) VecDuplicate(like, &k->work[q]);
    else lz_before_write(k->work[q], 1);
    return k->work[q];
}
static void swap_dev(Vec a, Vec b) { double *t = a->dev; a->dev = b->dev; b->dev = t; }

/* ---- PCMG application and the outer Richardson of -cycle 8 ---- */
static Vec mg_vec(Vec *slot, unsigned char *own, Mat A, int want_rows) {
    if (!*slot) {                                   /* not provided through PCMGSetRhs/X/R: create it */
        if (want_rows) MatCreateVecs(A, NULL, slot); else MatCreateVecs(A, slot, NULL);
        *own = 1;
    }
    return *slot;
}
static void mg_setup(KSP k) {
    pcmg *mg = k->pcobj.mg;
    static int noted = 0;
    for (int i = 0; i < mg->levels; i++) {
        KSP s = mg->smooth[i];
        if (!s->A) { fprintf(stderr, "[mgpetsc] FATAL: PCMG level %d has no operators (KSPSetOperators on PCMGGetSmoother/CoarseSolve)\n", i); exit(86); }
        if (i > 0 && (!mg->interp[i] || !mg->restr[i])) { fprintf(stderr, "[mgpetsc] FATAL: PCMG level %d lacks interpolation/restriction\n", i); exit(86); }
        if (!s->type_from_user && i == 0 && s->pc == P_DEFAULT && s->A->m <= MGP_LU_MAX) {
            s->type = K_PREONLY; s->pc = P_LU;           /* PETSc's default coarse solver: preonly + LU, an exact solve */
        } else if (!s->type_from_user) {
            if (!noted) {
                fprintf(stderr, "[mgpetsc] note: PCMG's PETSc default smoother (chebyshev + SOR with estimated eigenvalues) is not provided; "
                                "level solvers without -mg_levels_ksp_type use richardson + jacobi, %d sweeps (the default coarse solve is "
                                "exact, as PETSc's preonly + LU, up to 1024 unknowns)\n", (int)s->maxits);
                noted = 1;
            }
            s->type = K_RICHARDSON;
            if (s->pc == P_DEFAULT) s->pc = P_JACOBI;
        }
        if (s->pc == P_MG) UNSUPPORTED("nested PCMG");
        s->normtype = KSP_NORM_NONE;
        s->guess_nonzero = (i > 0);
        if (i < mg->levels - 1) {                       /* the finest level's b and x are the arguments of the application */
            mg_vec(&mg->b[i], &mg->own_b[i], s->A, 1);
            mg_vec(&mg->x[i], &mg->own_x[i], s->A, 0);
        }
        if (i > 0) mg_vec(&mg->r[i], &mg->own_r[i], s->A, 1);
    }
}
static int mg_tail_try(pcmg *mg, int i, Vec b, Vec x);     /* levels 0 .. i as ONE tail launch (below, with the recorder) */
static void mg_cycle(pcmg *mg, int i, Vec b, Vec x) {       /* PCMGMCycle_Private, one cycle per level */
    KSP s = mg->smooth[i];
    if (i == 0) { KSPSolve(s, b, x); return; }            /* coarse solve (zero initial guess) */
    if (mg_tail_try(mg, i, b, x)) return;
    {   /* pre-smoothing: x is the zero vector on entry (the caller's x_i = 0), so the solve runs with the zero-guess flag -- the same
         * values (0 + s*((b - 0)*dinv) is the zero-guess sweep bit for bit) without the zero fill and without reading x, and the first
         * sweep can come out of the restriction's pass */
        const int g = s->guess_nonzero;
        s->guess_nonzero = 0;
        KSPSolve(s, b, x);
        s->guess_nonzero = g;
    }
    MatResidual(s->A, b, x, mg->r[i]);
    MatMult(mg->restr[i], mg->r[i], mg->b[i - 1]);          /* MatRestrict; x_{i-1} = 0 is implied by the zero-guess solve below */
    if (mg->r[i]->lz) { g_lzstat[5]++; lz_drop(mg->r[i]); }  /* PCMG's residual work vector (PCMGSetR): consumed by the fused restriction, its
                                                              * contents after the cycle are unspecified -- not computed when x changes below */
    mg_cycle(mg, i - 1, mg->b[i - 1], mg->x[i - 1]);
    MatMultAdd(mg->interp[i], mg->x[i - 1], x, x);          /* MatInterpolateAdd */
    KSPSolve(s, b, x);                                      /* post-smoothing */
}
/* KSPSolve of the outer solver (src/solver.c:1963): Richardson, x += scale * M^{-1} r, unpreconditioned residual
 * norm logged to the residual history, KSPConvergedDefault (rtol * ||b|| with a zero guess, atol, dtol). */
static PetscErrorCode ksp_solve_mg(KSP k, Vec b, Vec x) {
    Mat A = k->A;
    pcmg *mg = k->pcobj.mg;
    if (!mg) UNSUPPORTED("KSPSolve with PCMG before PCMGSetLevels");
    if (k->type != K_RICHARDSON) UNSUPPORTED("PCMG under an outer Krylov type other than richardson");
    need_same(b, x, "KSPSolve");
    mg_setup(k);
    g_tc_off++;                                              /* (PCMG's own cycle calls MatMultAdd, not the reference loop's pattern: no recording) */
    k->b = b; k->x = x; k->its = 0;
    (void)vdev(b); (void)vdev(x);
    Vec r = ksp_work(k, 0, x), z = ksp_work(k, 1, x);
    if (!k->guess_nonzero) { VecSet(x, 0.0); VecCopy(b, r); }
    else MatResidual(A, b, x, r);
    PetscReal rn = 0.0, rn0;
    VecNorm(r, NORM_2, &rn);
    rn0 = rn;
    if (k->hist && k->nhist > 0) k->hist[0] = rn;
    double ttol = k->rtol * rn0;
    if (ttol < k->atol) ttol = k->atol;
    const int top = mg->levels - 1;
    while (k->its < k->maxits && rn > ttol && !(rn >= k->dtol * rn0) && rn == rn) {
        if (top == 0) VecSet(z, 0.0);
        mg_cycle(mg, top, r, z);                                                /* z = M^{-1} r (from z = 0: zero-guess solves) */
        VecAXPY(x, k->scale, z);
        MatResidual(A, b, x, r);
        VecNorm(r, NORM_2, &rn);
        k->its++;
        if (k->hist && k->its < k->nhist) k->hist[k->its] = rn;
    }
    g_tc_off--;
    return 0;
}

/* KSPSolve with KSP_NORM_UNPRECONDITIONED and an ordinary PC: the single-level iteration of -cycle 1
 * (MultigridIcycle, src/solver.c:1991-2060): x += scale * B (b - A x), ||b - A x||_2 logged after every iteration,
 * KSPConvergedDefault's test.  One sweep at a time through the KSP_NORM_NONE path below, so the arithmetic is the
 * smoother's. */
static PetscErrorCode ksp_solve_monitored(KSP k, Vec b, Vec x) {
    Mat A = k->A;
    if (k->type != K_RICHARDSON) UNSUPPORTED("a monitored (KSP_NORM_UNPRECONDITIONED) solve with a Krylov type other than richardson");
    need_same(b, x, "KSPSolve");
    g_tc_off++;                                              /* (one sweep per inner solve with a norm in between: nothing to record) */
    const PetscInt maxits = k->maxits;
    const int guess = k->guess_nonzero;
    Vec r = ksp_work(k, 2, x);
    (void)vdev(b); (void)vdev(x);
    if (!guess) { VecSet(x, 0.0); VecCopy(b, r); } else MatResidual(A, b, x, r);
    PetscReal rn = 0.0, rn0;
    VecNorm(r, NORM_2, &rn);
    rn0 = rn;
    if (k->hist && k->nhist > 0) k->hist[0] = rn;
    double ttol = k->rtol * rn0;
    if (ttol < k->atol) ttol = k->atol;
    PetscInt its = 0;
    k->normtype = KSP_NORM_NONE; k->maxits = 1;
    while (its < maxits && rn > ttol && !(rn >= k->dtol * rn0) && rn == rn) {
        k->guess_nonzero = (guess || its > 0);
        KSPSolve(k, b, x);
        MatResidual(A, b, x, r);
        VecNorm(r, NORM_2, &rn);
        its++;
        if (k->hist && its < k->nhist) k->hist[its] = rn;
    }
    k->normtype = KSP_NORM_UNPRECONDITIONED; k->maxits = maxits; k->guess_nonzero = guess; k->its = its;
    k->b = b; k->x = x;
    g_tc_off--;
    return 0;
}

/* PCLU (with any KSP type): x = A^-1 b.  PETSc factors; this drop-in inverts the small matrix once on the host (Gauss-Jordan with
 * partial pivoting on the assembled values) and applies the dense inverse on the GPU (mgk_dense_mult_f64) -- the same exact solve
 * up to rounding.  Meant for PCMG's coarsest grid (PETSc's default coarse solver, src/solver.c:1931-1932): at most 1024 unknowns. */
static void mat_device_inverse(Mat A) {
    if (A->d_inv && !A->inv_stale) return;
    const int m = A->m;
    double *M = (double *)calloc((size_t)m * 2 * m, sizeof(double));
    if (!M) { fprintf(stderr, "[mgpetsc] FATAL: out of memory (dense inverse)\n"); exit(88); }
    const int w = 2 * m;
    for (int r = 0; r < m; r++) {
        for (long q = A->rowptr[r]; q < A->rowptr[r + 1]; q++) M[(size_t)r * w + A->col[q]] += A->val[q];
        M[(size_t)r * w + m + r] = 1.0;
    }
    for (int c = 0; c < m; c++) {
        int p = c;
        for (int r = c + 1; r < m; r++) if (fabs(M[(size_t)r * w + c]) > fabs(M[(size_t)p * w + c])) p = r;
        if (M[(size_t)p * w + c] == 0.0) { fprintf(stderr, "[mgpetsc] FATAL: PCLU: the matrix is singular\n"); exit(88); }
        if (p != c) for (int j = 0; j < w; j++) { double t = M[(size_t)p * w + j]; M[(size_t)p * w + j] = M[(size_t)c * w + j]; M[(size_t)c * w + j] = t; }
        const double d = 1.0 / M[(size_t)c * w + c];
        for (int j = c; j < w; j++) M[(size_t)c * w + j] *= d;
        for (int r = 0; r < m; r++) {
            if (r == c) continue;
            const double f = M[(size_t)r * w + c];
            if (f == 0.0) continue;
            for (int j = c; j < w; j++) M[(size_t)r * w + j] -= f * M[(size_t)c * w + j];
        }
    }
    double *inv = (double *)malloc(sizeof(double) * (size_t)m * m);
    for (int r = 0; r < m; r++) memcpy(inv + (size_t)r * m, M + (size_t)r * w + m, sizeof(double) * (size_t)m);
    free(M);
    void *p;
    if (!A->d_inv) {
        DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)m * m)); A->d_inv = (double *)p;
        DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)(m < 16 ? 16 : m))); A->d_c1 = (double *)p;
        DEV(mgk_malloc(G, &p, sizeof(double) * (size_t)(m < 16 ? 16 : m))); A->d_c2 = (double *)p;
    }
    DEV(mgk_h2d(G, A->d_inv, inv, sizeof(double) * (size_t)m * m));
    free(inv);
    A->inv_stale = 0;
}
/* x = A^-1 b with the dense inverse (x is overwritten) */
static void direct_apply(Mat A, Vec b, Vec x) {
    mat_device_inverse(A);
    const double *bd = vdev(b);
    lz_before_write(x, 1);
    x->host_dirty = 0;
    if (b->padded) {
        DEV(mgk_unpack_f64(G, &b->g, bd, A->d_c1, NULL));
        DEV(mgk_dense_mult_f64(G, A->m, A->m, A->d_inv, A->d_c1, A->d_c2, NULL));
        DEV(mgk_pack_f64(G, &x->g, A->d_c2, x->dev, NULL));
    } else DEV(mgk_dense_mult_f64(G, A->m, A->m, A->d_inv, bd, x->dev, NULL));
}
/* -pc_type lu.  With an exact preconditioner B = A^-1:
 *   preonly, and every Krylov method PETSc would default to (exact after one step): x = A^-1 b;
 *   richardson, scale 1, max_it >= 1: x_1 = x_0 + 1 * A^-1 (b - A x_0) = A^-1 b whatever the guess: the same;
 *   richardson, scale s != 1 (or max_it = 0): x_{k+1} = x_k + s A^-1 (b - A x_k) = (1 - s) x_k + s y with y = A^-1 b, i.e. after
 *     m = max_it steps  x_m = (1 - s)^m x_0 + (1 - (1 - s)^m) y  (x_0 = 0 without KSPSetInitialGuessNonzero) -- NOT an exact solve,
 *     and PETSc would not make it one (it used to be returned as exact, silently);
 *   chebyshev + lu: not provided. */
static PetscErrorCode ksp_solve_direct(KSP k, Vec b, Vec x) {
    Mat A = k->A;
    if (A->m != A->n) UNSUPPORTED("PCLU on a rectangular operator");
    if (A->m > MGP_LU_MAX) UNSUPPORTED("PCLU on more than 1024 unknowns (it is meant for PCMG's coarsest grid: use more levels)");
    need_same(b, x, "KSPSolve");
    if (b->padded == 2 || b == x) UNSUPPORTED("PCLU on a several-grid level operator / in place");
    if (k->type == K_CHEBYSHEV) UNSUPPORTED("-ksp_type chebyshev with -pc_type lu (use preonly or richardson)");
    k->b = b; k->x = x;
    if (k->type == K_RICHARDSON && (k->scale != 1.0 || k->maxits < 1)) {
        Vec y = NULL;
        VecDuplicate(x, &y);
        direct_apply(A, b, y);
        const double c = pow(1.0 - k->scale, (double)k->maxits);        /* weight of the initial guess after max_it damped steps */
        if (k->guess_nonzero) VecScale(x, c); else VecSet(x, 0.0);
        VecAXPY(x, 1.0 - c, y);
        VecDestroy(&y);
        k->its = k->maxits;
        return 0;
    }
    direct_apply(A, b, x);
    k->its = 1;
    return 0;
}

/* round 3: Richardson solves of >= 3 sweeps on 2-D stencil operators start with ONE pass that makes three of them (mgk_jacobi3_2d_*): over b
 * alone from the zero guess, with the prolongation when the guess is u + P u_c still deferred, with the residual norm when the solve opens
 * the next cycle.  MGPETSC_J3=0 keeps the round-2 sequence (first sweep fused with its producer, the others one or two per pass). */
static int j3_on(void) {
    static int v = -1;
    if (v < 0) { const char *e = getenv("MGPETSC_J3"); v = (e && *e) ? atoi(e) : 1; }
    return v;
}

/* ---- tail capture (round 3) -------------------------------------------------------------------------------------------------------
 * Below 63^2 a level's part of the reference's loop (src/solver.c:1533-1544) is three launches of ~5 us whose arithmetic is a rounding
 * error; the own driver runs those levels as ONE launch of one workgroup with everything in LDS (mgk_tail_cycle_f64).  The drop-in sees
 * the same work as a stream of PETSc calls, so it RECORDS them instead of executing them, as long as they keep to the pattern
 *     KSPSolve(ksp[t], b[t], u[t])                                  zero guess, n <= 63: the recording starts (b[t] is made concrete)
 *     { KSPBuildResidual / MatResidual(A[l], b[l], u[l], r[l]);  MatMult(res[l], r[l], b[l+1]);  KSPSolve(ksp[l+1], b[l+1], u[l+1]) }   l = t, t+1, ...
 *     { MatMult(pro[l], u[l+1], rv[l]);  VecAXPY(u[l], 1.0, rv[l]);  KSPSolve(ksp[l], b[l], u[l]) }                                     ... back up to l = t
 * (Richardson, Jacobi / none, one scale, max_it = v0 above the coarsest level; the solver's parameters are snapshot at each call, so the
 * KSPSetInitialGuessNonzero calls in between, :1537 and :1543, need nothing).  When the last call of the pattern arrives the tail kernel
 * runs the whole sub-cycle and u[t] is concrete; the intermediates (u, b, r, rv of the levels below) are never computed -- they stay marked
 * LZ_TAIL with the log kept, and the next cycle overwrites them unread.  PETSc's semantics hold for everything else: the vectors a recording
 * has written are LZ_TAIL, so ANY read of one (vdev -> lz_settle), any write to one or to b[t] (lz_before_write), any change or destruction
 * of a matrix or solver the log names, and any of the four intercepted calls that does not continue the pattern first REPLAYS the log call
 * by call through the ordinary paths (tc_flush); an intermediate of a finished sub-cycle that is read after all is computed by replaying
 * the log on scratch vectors (tc_materialise: the real ones may hold newer values by then).  MGPETSC_TAIL=0 switches the recorder off. */
#define TC_MAXLEV 8
enum { TC_SOLVE = 1, TC_RESID, TC_RESTRICT, TC_PROLONG, TC_AXPY, TC_MULTADD };
enum { TCS_AFTER_PRE = 1, TCS_AFTER_RESID, TCS_AFTER_RESTRICT, TCS_AFTER_PROLONG, TCS_AFTER_AXPY, TCS_AFTER_POST };
typedef struct { int op; KSP k; Mat A; Vec a, b, c; int guess, pc, type; PetscInt maxits; double scale; KSPNormType nt; } tc_op;
typedef struct {
    int complete;                                   /* 0: recording; 1: the tail kernel has run, the intermediates are unread ghosts */
    int nops; tc_op ops[6 * TC_MAXLEV + 2];
    int nlev, j, step;                              /* levels entered so far, current level, what the last absorbed call was */
    KSP ksp[TC_MAXLEV]; Mat A[TC_MAXLEV], R[TC_MAXLEV], P[TC_MAXLEV];
    Vec b[TC_MAXLEV], u[TC_MAXLEV], r[TC_MAXLEV], rv[TC_MAXLEV];
    PetscInt its[TC_MAXLEV]; int pc[TC_MAXLEV]; double scale;
    int nv; Vec vec[4 * TC_MAXLEV]; mgk_geom vg[4 * TC_MAXLEV]; PetscInt vn[4 * TC_MAXLEV]; char alive[4 * TC_MAXLEV];   /* the vectors the log writes */
    double *b0_priv; long b0_n;                     /* finished log: its right-hand side, once b[0] itself has been given a new value (below) */
    mgk_geom b0_g; PetscInt b0_len;
} tailcap;
static tailcap *g_tc_rec = NULL, *g_tc_done = NULL;
/* The reference overwrites b[t] (MatMult(res), :1535) BEFORE it overwrites the intermediates of the previous cycle, and those are defined in
 * terms of the old b[t].  Computing them at that point would double the work, copying b[t] would cost a launch per cycle: instead the log
 * takes b[t]'s device buffer (its old value is dead for the vector: the write is a full overwrite) and the vector continues on a spare buffer
 * of the same layout -- the buffer the previous log gave back when its last ghost was overwritten.  A partial write copies. */
static double *g_tc_spare = NULL; static long g_tc_spare_n = 0;
static void tc_free_log(tailcap *t) {
    if (t->b0_priv) {
        if (g_tc_spare && G) mgk_free(G, g_tc_spare);
        g_tc_spare = t->b0_priv; g_tc_spare_n = t->b0_n;
    }
    free(t);
}
static void tc_input_changing(Vec v, int full) {
    tailcap *t = g_tc_done;
    if (!t || v != t->b[0] || t->b0_priv) return;
    double *spare = NULL;
    if (g_tc_spare && g_tc_spare_n == v->nalloc) { spare = g_tc_spare; g_tc_spare = NULL; g_tc_spare_n = 0; }
    else {
        void *q = NULL;
        DEV(mgk_malloc(G, &q, sizeof(double) * (size_t)v->nalloc));
        DEV(mgk_memset0(G, q, sizeof(double) * (size_t)v->nalloc, NULL));       /* (the padding of the layout is zero and stays zero) */
        spare = (double *)q;
    }
    if (v->host_dirty) vec_upload(v);
    if (full) { t->b0_priv = v->dev; v->dev = spare; }
    else { DEV(mgk_d2d(G, spare, v->dev, sizeof(double) * (size_t)v->nalloc, NULL)); t->b0_priv = spare; }
    t->b0_n = v->nalloc; t->b0_g = v->g; t->b0_len = v->n;
    for (int i = 0; i < t->nv; i++) if (t->alive[i]) t->vec[i]->lz_b = NULL;        /* the ghosts no longer depend on the vector */
}
static int tc_on(void) {
    static int v = -1;
    if (v < 0) { const char *e = getenv("MGPETSC_TAIL"); v = (e && *e) ? atoi(e) : 1; }
    return v && lazy_on() == 1 && g_tc_off == 0;
}
static int tc_index(const tailcap *t, Vec v) { for (int i = 0; t && i < t->nv; i++) if (t->vec[i] == v) return i; return -1; }
static int tc_recording_has(Vec v) { return g_tc_rec && tc_index(g_tc_rec, v) >= 0; }
static void tc_unmark(Vec v) {                                      /* (lz_drop without the bookkeeping of a dropped ghost) */
    if (v->lz != LZ_TAIL) return;
    v->lz = LZ_NONE; v->lz_A = v->lz_A2 = NULL; v->lz_b = v->lz_x = NULL; v->lz_ksp = NULL;
    for (int q = 0; q < g_nlz; q++) if (g_lz[q] == v) { g_lz[q] = g_lz[--g_nlz]; break; }
}
/* v becomes a vector the recording writes (every one of them fully, the first time) */
static void tc_take(tailcap *t, Vec v) {
    if (tc_index(t, v) >= 0) return;                                /* (r[l] and rv[l] are one vector in the reference) */
    lz_before_write(v, 1);                                          /* its old value dies: dependents computed, an older deferred value / ghost dropped */
    v->host_dirty = 0;
    t->vec[t->nv] = v; t->vg[t->nv] = v->g; t->vn[t->nv] = v->n; t->alive[t->nv] = 1; t->nv++;
    lz_register(v, LZ_TAIL, NULL, t->b[0], NULL);                   /* depends on the sub-cycle's right-hand side */
}
static void tc_log(tailcap *t, int op, KSP k, Mat A, Vec a, Vec b, Vec c) {
    tc_op *o = &t->ops[t->nops++];
    memset(o, 0, sizeof(*o));
    o->op = op; o->k = k; o->A = A; o->a = a; o->b = b; o->c = c;
    if (k) { o->guess = k->guess_nonzero; o->pc = (k->pc == P_LU) ? P_LU : ksp_pc(k); o->type = k->type; o->maxits = k->maxits; o->scale = k->scale; o->nt = k->normtype; }
}
/* one logged call through the ordinary paths, on (possibly substituted) vectors */
static void tc_run(const tc_op *o, Vec a, Vec b, Vec c) {
    switch (o->op) {
    case TC_SOLVE: {
        KSP k = o->k;
        Mat A0 = k->A; const int g0 = k->guess_nonzero, t0 = k->type, p0 = k->pc; const PetscInt m0 = k->maxits, i0 = k->its; const double s0 = k->scale;
        const KSPNormType n0 = k->normtype; Vec kb = k->b, kx = k->x;
        k->A = o->A; k->guess_nonzero = o->guess; k->type = o->type; k->pc = o->pc; k->maxits = o->maxits; k->scale = o->scale; k->normtype = o->nt;
        KSPSolve(k, a, b);
        k->A = A0; k->guess_nonzero = g0; k->type = t0; k->pc = p0; k->maxits = m0; k->scale = s0; k->normtype = n0; k->its = i0;
        if (a != o->a || b != o->b) { k->b = kb; k->x = kx; }           /* scratch vectors: the solver keeps naming the real ones */
        break;
    }
    case TC_RESID: MatResidual(o->A, a, b, c); break;
    case TC_RESTRICT: case TC_PROLONG: MatMult(o->A, a, b); break;
    case TC_AXPY: VecAXPY(a, 1.0, b); break;
    case TC_MULTADD: MatMultAdd(o->A, a, b, b); break;           /* MatInterpolateAdd of PCMG's own cycle */
    }
}
/* the recording is executed after all, call by call, on the real vectors */
static void tc_flush(void) {
    tailcap *t = g_tc_rec;
    if (!t) return;
    g_tc_rec = NULL;
    g_lzstat[12]++;
    for (int i = 0; i < t->nv; i++) tc_unmark(t->vec[i]);
    g_tc_off++;
    for (int q = 0; q < t->nops; q++) tc_run(&t->ops[q], t->ops[q].a, t->ops[q].b, t->ops[q].c);
    g_tc_off--;
    tc_free_log(t);
}
/* an intermediate of a finished sub-cycle is read after all: the log is replayed on scratch vectors (the real u[t], and any intermediate the
 * caller has overwritten since, hold newer values) and the intermediates that are still unread ghosts receive their values */
static void tc_materialise(void) {
    tailcap *t = g_tc_done;
    if (!t) return;
    g_tc_done = NULL;
    g_lzstat[13]++;
    if (getenv("MGPETSC_TAIL_DEBUG")) {
        fprintf(stderr, "[mgpetsc] tail log of %d levels from n = %d: intermediates computed after all; unread so far:", t->nlev, t->A[0]->gf.nx);
        for (int i = 0; i < t->nv; i++) if (t->alive[i]) fprintf(stderr, " vec#%d(n=%d)", i, (int)t->vn[i]);
        fprintf(stderr, "\n");
    }
    Vec tmp[4 * TC_MAXLEV], tb0 = NULL;
    for (int i = 0; i < t->nv; i++) tmp[i] = vec_new(t->vn[i], &t->vg[i]);
    if (t->b0_priv) {                                               /* the right-hand side as it was (b[0] itself has a newer value) */
        tb0 = vec_new(t->b0_len, &t->b0_g);
        DEV(mgk_d2d(G, tb0->dev, t->b0_priv, sizeof(double) * (size_t)t->b0_n, NULL));
    }
    g_tc_off++;
#define TC_MAP(v) (tc_index(t, (v)) >= 0 ? tmp[tc_index(t, (v))] : ((v) == t->b[0] && tb0) ? tb0 : (v))
    for (int q = 0; q < t->nops; q++) {
        const tc_op *o = &t->ops[q];
        tc_run(o, o->a ? TC_MAP(o->a) : NULL, o->b ? TC_MAP(o->b) : NULL, o->c ? TC_MAP(o->c) : NULL);
    }
#undef TC_MAP
    for (int i = 0; i < t->nv; i++) {
        if (t->alive[i]) {
            Vec v = t->vec[i];
            tc_unmark(v);
            v->host_dirty = 0; v->ver++;
            DEV(mgk_d2d(G, v->dev, vdev(tmp[i]), sizeof(double) * (size_t)v->nalloc, NULL));
        }
    }
    for (int i = 0; i < t->nv; i++) VecDestroy(&tmp[i]);
    if (tb0) VecDestroy(&tb0);
    g_tc_off--;
    tc_free_log(t);
}
static void tc_settle(Vec v) {
    if (tc_recording_has(v)) tc_flush();
    else if (g_tc_done && tc_index(g_tc_done, v) >= 0) tc_materialise();
    else tc_unmark(v);                                              /* (cannot happen: a LZ_TAIL vector belongs to one of the two logs) */
}
static void tc_dropped(Vec v) {                                     /* a ghost overwritten unread; the log goes with the last of them */
    tailcap *t = g_tc_done;
    const int i = tc_index(t, v);
    if (i < 0) return;
    t->alive[i] = 0;
    for (int q = 0; q < t->nv; q++) if (t->alive[q]) return;
    g_tc_done = NULL;
    tc_free_log(t);
}
static int tc_names_mat(const tailcap *t, Mat A) {
    for (int l = 0; t && l < t->nlev; l++) if (t->A[l] == A || t->R[l] == A || t->P[l] == A) return 1;
    return 0;
}
static void tc_mat_changing(struct _p_Mat *A) {
    if (tc_names_mat(g_tc_rec, A)) tc_flush();
    if (tc_names_mat(g_tc_done, A)) tc_materialise();
}
static void tc_ksp_dying(KSP k) {
    for (int l = 0; g_tc_rec && l < g_tc_rec->nlev; l++) if (g_tc_rec->ksp[l] == k) { tc_flush(); break; }
    for (int l = 0; g_tc_done && l < g_tc_done->nlev; l++) if (g_tc_done->ksp[l] == k) { tc_materialise(); break; }
}
static void tc_shutdown(void) {                                     /* PetscFinalize: nobody reads anything any more */
    tailcap *both[2] = {g_tc_rec, g_tc_done};
    g_tc_rec = g_tc_done = NULL;
    for (int q = 0; q < 2; q++) if (both[q]) { for (int i = 0; i < both[q]->nv; i++) if (q == 0 || both[q]->alive[i]) tc_unmark(both[q]->vec[i]); tc_free_log(both[q]); }
    if (g_tc_spare && G) mgk_free(G, g_tc_spare);
    g_tc_spare = NULL; g_tc_spare_n = 0;
}
static int tc_level_ok(Mat A, Vec b, Vec x) {                       /* a level the tail kernel handles, on vectors in the padded layout */
    return (A->kind == MAT_STENCIL || A->kind == MAT_STENCIL_ROW) && A->gf.dim == 2 && A->gf.nx == A->gf.ny && A->gf.nx <= mgk_tail_max_n(2) &&
           b->padded == 1 && x->padded == 1 && geom_eq(&b->g, &A->gf) && geom_eq(&x->g, &A->gf) && b != x;
}
/* the last call of the pattern has arrived: ONE launch for the whole sub-cycle */
static void tc_complete(tailcap *t) {
    int n[TC_MAXLEV];
    double coef7[7 * TC_MAXLEV], dinv[TC_MAXLEV];
    const double *ctab[TC_MAXLEV], *dtab[TC_MAXLEV];
    const int rows = t->A[0]->kind == MAT_STENCIL_ROW;
    for (int l = 0; l < t->nlev; l++) {
        Mat A = t->A[l];
        n[l] = A->gf.nx;
        if (rows) { mat_device_rowtabs(A); ctab[l] = A->d_ctab; dtab[l] = (t->pc[l] == P_JACOBI) ? A->d_dtab : A->d_ones; }
        else {
            for (int q = 0; q < 7; q++) coef7[7 * l + q] = q < 5 ? A->coef[q] : 0.0;
            dinv[l] = (t->pc[l] == P_JACOBI) ? 1.0 / A->coef[2] : 1.0;
        }
    }
    Vec b0 = t->b[0], u0 = t->u[0];
    const int v0 = (int)t->its[0], v1 = (int)t->its[t->nlev - 1];
    g_tc_rec = NULL;
    tc_unmark(u0);                                                  /* written in full by the kernel below: concrete from here on */
    t->alive[tc_index(t, u0)] = 0;
    u0->host_dirty = 0; u0->ver++;
    if (rows) DEV(mgk_tail_cycle_rowcoef_f64(G, &u0->g, t->nlev, n, ctab, dtab, t->scale, v0, v1, b0->dev, u0->dev, NULL));
    else DEV(mgk_tail_cycle_f64(G, &u0->g, t->nlev, n, coef7, dinv, t->scale, v0, v1, b0->dev, u0->dev, NULL));
    g_lzstat[11]++;
    t->complete = 1;
    if (g_tc_done) tc_materialise();                                /* (an older finished log whose ghosts this cycle did not overwrite: rare) */
    int any = 0;
    for (int i = 0; i < t->nv; i++) any |= t->alive[i];
    if (any) g_tc_done = t; else tc_free_log(t);
}
/* KSPSolve asks here first (Richardson, KSP_NORM_NONE, max_it >= 1, operands checked): 1 = absorbed */
static int tc_solve(KSP k, Vec b, Vec x) {
    Mat A = k->A;
    tailcap *t = g_tc_rec;
    if (t) {
        const int j = t->j;
        if (t->step == TCS_AFTER_RESTRICT && !k->guess_nonzero && b == t->b[j + 1] && tc_index(t, x) < 0 && tc_level_ok(A, b, x) &&
            A->kind == t->A[0]->kind && A->gf.nx == (t->A[j]->gf.nx - 1) / 2 && k->scale == t->scale && k->maxits >= 1 && j + 2 <= TC_MAXLEV) {
            int fresh = 1;
            for (int l = 0; l <= j; l++) if (t->ksp[l] == k) fresh = 0;
            if (fresh) {
                t->j = j + 1; t->nlev = j + 2;
                t->ksp[j + 1] = k; t->A[j + 1] = A; t->u[j + 1] = x; t->its[j + 1] = k->maxits; t->pc[j + 1] = ksp_pc(k);
                tc_take(t, x);
                tc_log(t, TC_SOLVE, k, A, b, x, NULL);
                t->step = TCS_AFTER_PRE;
                k->b = b; k->x = x; k->its = k->maxits;
                return 1;
            }
        }
        if (t->step == TCS_AFTER_AXPY && k->guess_nonzero && k == t->ksp[j] && A == t->A[j] && b == t->b[j] && x == t->u[j] &&
            k->maxits == t->its[0] && k->scale == t->scale && ksp_pc(k) == t->pc[j]) {
            tc_log(t, TC_SOLVE, k, A, b, x, NULL);
            k->b = b; k->x = x; k->its = k->maxits;
            if (j == 0) tc_complete(t); else t->step = TCS_AFTER_POST;
            return 1;
        }
        tc_flush();
    }
    /* a pre-smoothing solve from the zero guess on a level the tail kernel holds: a recording starts */
    if (!tc_on() || k->guess_nonzero || k->maxits < 1 || !tc_level_ok(A, b, x) || A->gf.nx < 3) return 0;
    (void)vdev(b);                                                   /* the sub-cycle's right-hand side: concrete, on the device */
    t = (tailcap *)calloc(1, sizeof(*t));
    if (!t) return 0;
    t->nlev = 1; t->j = 0; t->step = TCS_AFTER_PRE;
    t->ksp[0] = k; t->A[0] = A; t->b[0] = b; t->u[0] = x; t->its[0] = k->maxits; t->pc[0] = ksp_pc(k); t->scale = k->scale;
    tc_take(t, x);
    g_tc_rec = t;
    tc_log(t, TC_SOLVE, k, A, b, x, NULL);
    k->b = b; k->x = x; k->its = k->maxits;
    return 1;
}
static int tc_resid(struct _p_Mat *A, Vec b, Vec x, Vec r) {
    tailcap *t = g_tc_rec;
    if (!t) return 0;
    const int j = t->j;
    if (t->step == TCS_AFTER_PRE && A == t->A[j] && b == t->b[j] && x == t->u[j] && r != b && r != x && r->padded == 1 && geom_eq(&r->g, &A->gf) &&
        (tc_index(t, r) < 0) && j + 1 < TC_MAXLEV) {
        t->r[j] = r;
        tc_take(t, r);
        tc_log(t, TC_RESID, NULL, A, b, x, r);
        t->step = TCS_AFTER_RESID;
        return 1;
    }
    tc_flush();
    return 0;
}
static int tc_mult(struct _p_Mat *A, Vec x, Vec y) {
    tailcap *t = g_tc_rec;
    if (!t) return 0;
    const int j = t->j;
    if (A->kind == MAT_RESTRICT && t->step == TCS_AFTER_RESID && x == t->r[j] && geom_eq(&A->gf, &t->A[j]->gf) && A->gc.nx == (A->gf.nx - 1) / 2 &&
        A->gc.nx >= 1 && y->padded == 1 && geom_eq(&y->g, &A->gc) && tc_index(t, y) < 0 && y != t->b[0]) {
        t->R[j] = A; t->b[j + 1] = y;
        tc_take(t, y);
        tc_log(t, TC_RESTRICT, NULL, A, x, y, NULL);
        t->step = TCS_AFTER_RESTRICT;
        return 1;
    }
    if (A->kind == MAT_PROLONG && j >= 1 && (t->step == TCS_AFTER_PRE || t->step == TCS_AFTER_POST) && x == t->u[j] && geom_eq(&A->gc, &t->A[j]->gf) &&
        geom_eq(&A->gf, &t->A[j - 1]->gf) && y->padded == 1 && geom_eq(&y->g, &A->gf) && y != t->u[j - 1] && y != t->b[j - 1]) {
        int ok = 1;
        if (t->step == TCS_AFTER_PRE) for (int l = 0; l < j; l++) if (t->its[l] != t->its[0]) ok = 0;       /* the turn: level j is the coarsest; v0 above it */
        if (ok) {
            t->P[j - 1] = A; t->rv[j - 1] = y;
            tc_take(t, y);
            tc_log(t, TC_PROLONG, NULL, A, x, y, NULL);
            t->j = j - 1; t->step = TCS_AFTER_PROLONG;
            return 1;
        }
    }
    tc_flush();
    return 0;
}
static int tc_axpy(Vec y, double a, Vec x) {
    tailcap *t = g_tc_rec;
    if (!t) return 0;
    if (t->step == TCS_AFTER_PROLONG && a == 1.0 && y == t->u[t->j] && x == t->rv[t->j]) {
        tc_log(t, TC_AXPY, NULL, NULL, y, x, NULL);
        t->step = TCS_AFTER_AXPY;
        return 1;
    }
    tc_flush();
    return 0;
}

/* PCMG's own cycle (-cycle 8) on the levels 0 .. i, x = cycle(b) from x = 0, as ONE tail launch: every level a 2-D stencil operator of
 * n <= 63 with the canonical transfer operators; Richardson + Jacobi / none with one damping factor and one max_it on the levels above the
 * coarsest; the coarsest solved by Richardson too, by one undamped step (preonly), or exactly -- PETSc's default, LU -- on a 1 x 1 grid, where the
 * exact solve IS one undamped Jacobi sweep from the zero guess.  The level vectors below i (the reference hands PCMG its own through
 * PCMGSetRhs / PCMGSetX, src/solver.c:1949-1954) are not computed: they become LZ_TAIL ghosts of a finished log that holds the calls of
 * mg_cycle, computed on scratch vectors if anybody reads them (tc_materialise), dropped when the next cycle overwrites them. */
static int mg_tail_try(pcmg *mg, int i, Vec b, Vec x) {
    static int on = -1;
    if (on < 0) { const char *e = getenv("MGPETSC_TAIL"); on = (e && *e) ? atoi(e) : 1; }
    if (!on || lazy_on() != 1 || i < 1 || i + 1 > TC_MAXLEV) return 0;
    KSP top = mg->smooth[i];
    if (!top->A || (top->A->kind != MAT_STENCIL && top->A->kind != MAT_STENCIL_ROW)) return 0;
    const int rows = top->A->kind == MAT_STENCIL_ROW;
    const double scale = top->scale;
    const PetscInt v0 = top->maxits;
    int n[TC_MAXLEV], v1 = 1;
    double coef7[7 * TC_MAXLEV], dinv[TC_MAXLEV], cscale = scale;
    const double *ctab[TC_MAXLEV], *dtab[TC_MAXLEV];
    if (b->padded != 1 || x->padded != 1 || b == x || !geom_eq(&b->g, &top->A->gf) || !geom_eq(&x->g, &top->A->gf)) return 0;
    for (int l = i; l >= 0; l--) {
        KSP s = mg->smooth[l];
        Mat A = s->A;
        const int t = i - l;                                         /* the tail counts from the finest level */
        if (!A || !A->assembled || A->kind != top->A->kind || A->gf.dim != 2 || A->gf.nx != A->gf.ny || A->gf.nx > mgk_tail_max_n(2)) return 0;
        if (t > 0 && A->gf.nx != (n[t - 1] - 1) / 2) return 0;
        n[t] = A->gf.nx;
        if (s->normtype == KSP_NORM_UNPRECONDITIONED || s->pc == P_MG || s->pc == P_DEFAULT) return 0;
        int jac = (s->pc == P_JACOBI);
        if (l > 0) {
            Mat R = mg->restr[l], P = mg->interp[l];
            Mat Ac = mg->smooth[l - 1]->A;
            if (s->type != K_RICHARDSON || s->scale != scale || s->maxits != v0 || v0 < 1 || (s->pc != P_JACOBI && s->pc != P_NONE)) return 0;
            if (!R || !P || !Ac || R->kind != MAT_RESTRICT || P->kind != MAT_PROLONG || !geom_eq(&R->gf, &A->gf) || !geom_eq(&P->gf, &A->gf) ||
                !geom_eq(&R->gc, &Ac->gf) || !geom_eq(&P->gc, &Ac->gf)) return 0;
            if (l < i && (!mg->x[l] || !mg->b[l] || mg->x[l]->padded != 1 || mg->b[l]->padded != 1 || !geom_eq(&mg->x[l]->g, &A->gf) ||
                          !geom_eq(&mg->b[l]->g, &A->gf) || mg->x[l] == mg->b[l])) return 0;
        } else {
            if (!mg->x[0] || !mg->b[0] || mg->x[0]->padded != 1 || mg->b[0]->padded != 1 || !geom_eq(&mg->x[0]->g, &A->gf) || !geom_eq(&mg->b[0]->g, &A->gf) ||
                mg->x[0] == mg->b[0]) return 0;
            if (s->pc == P_LU) {                                     /* exact: only where it is one undamped sweep */
                if (A->gf.nx != 1 || !(s->type == K_PREONLY || (s->type == K_RICHARDSON && s->scale == 1.0 && s->maxits >= 1))) return 0;
                v1 = 1; cscale = 1.0; jac = 1;
            } else if (s->type == K_PREONLY && (s->pc == P_JACOBI || s->pc == P_NONE)) { v1 = 1; cscale = 1.0; }
            else if (s->type == K_RICHARDSON && (s->pc == P_JACOBI || s->pc == P_NONE) && s->maxits >= 1) { v1 = (int)s->maxits; cscale = s->scale; }
            else return 0;
        }
        if (rows) { mat_device_rowtabs(A); ctab[t] = A->d_ctab; dtab[t] = jac ? A->d_dtab : A->d_ones; }
        else { for (int q = 0; q < 7; q++) coef7[7 * t + q] = q < 5 ? A->coef[q] : 0.0; dinv[t] = jac ? 1.0 / A->coef[2] : 1.0; }
    }
    /* the log of what mg_cycle would have called (replayed only if a ghost is read) */
    tailcap *t = (tailcap *)calloc(1, sizeof(*t));
    if (!t) return 0;
    (void)vdev(b);
    if (g_tc_done) {                                                 /* the previous cycle's ghosts are overwritten now: its log dies with them */
        for (int l = 0; l < i; l++) { lz_before_write(mg->x[l], 1); lz_before_write(mg->b[l], 1); }
        if (g_tc_done) tc_materialise();                             /* (another finished log: rare) */
    }
    t->complete = 1; t->nlev = i + 1; t->b[0] = b; t->u[0] = x; t->scale = scale;
    for (int l = i; l >= 0; l--) { t->ksp[i - l] = mg->smooth[l]; t->A[i - l] = mg->smooth[l]->A; if (l > 0) { t->R[i - l] = mg->restr[l]; t->P[i - l] = mg->interp[l]; } }
    lz_before_write(x, 1);
    x->host_dirty = 0; x->ver++;
#define MG_LOG_SOLVE(l_, rhs_, sol_, guess_) do { tc_log(t, TC_SOLVE, mg->smooth[l_], mg->smooth[l_]->A, (rhs_), (sol_), NULL); t->ops[t->nops - 1].guess = (guess_); } while (0)
    for (int l = i; l >= 1; l--) {                                   /* mg_cycle, level by level */
        Vec bl = (l == i) ? b : mg->b[l], xl = (l == i) ? x : mg->x[l];
        MG_LOG_SOLVE(l, bl, xl, 0);
        tc_log(t, TC_RESID, NULL, mg->smooth[l]->A, bl, xl, mg->r[l]);
        tc_log(t, TC_RESTRICT, NULL, mg->restr[l], mg->r[l], mg->b[l - 1], NULL);
    }
    MG_LOG_SOLVE(0, mg->b[0], mg->x[0], mg->smooth[0]->guess_nonzero);
    for (int l = 1; l <= i; l++) {
        Vec bl = (l == i) ? b : mg->b[l], xl = (l == i) ? x : mg->x[l];
        tc_log(t, TC_MULTADD, NULL, mg->interp[l], mg->x[l - 1], xl, NULL);
        MG_LOG_SOLVE(l, bl, xl, mg->smooth[l]->guess_nonzero);
    }
#undef MG_LOG_SOLVE
    /* the vectors the log writes: x (concrete after the launch), r[l] (PCMG's residual work vectors: contents unspecified after a cycle,
     * as in mg_cycle), and the ghosts x[l], b[l] below level i */
    t->vec[t->nv] = x; t->vg[t->nv] = x->g; t->vn[t->nv] = x->n; t->alive[t->nv] = 0; t->nv++;
    for (int l = i; l >= 1; l--) if (mg->r[l] && tc_index(t, mg->r[l]) < 0) {
        Vec r = mg->r[l];
        lz_before_write(r, 1);
        t->vec[t->nv] = r; t->vg[t->nv] = r->g; t->vn[t->nv] = r->n; t->alive[t->nv] = 0; t->nv++;
    }
    for (int l = i - 1; l >= 0; l--) { tc_take(t, mg->b[l]); tc_take(t, mg->x[l]); }
    if (rows) DEV(mgk_tail_cycle_cs_f64(G, &x->g, i + 1, n, NULL, NULL, ctab, dtab, scale, cscale, (int)v0, v1, b->dev, x->dev, NULL));
    else DEV(mgk_tail_cycle_cs_f64(G, &x->g, i + 1, n, coef7, dinv, NULL, NULL, scale, cscale, (int)v0, v1, b->dev, x->dev, NULL));
    g_lzstat[11]++;
    for (int l = 0; l <= i; l++) { mg->smooth[l]->its = (l == 0) ? v1 : v0; }
    mg->smooth[i]->b = b; mg->smooth[i]->x = x;
    for (int l = 0; l < i; l++) { mg->smooth[l]->b = mg->b[l]; mg->smooth[l]->x = mg->x[l]; }
    g_tc_done = t;
    return 1;
}

/* KSPSolve, KSP_NORM_NONE: exactly max_it iterations (src/solver.c:1531,1536,1542) */
PetscErrorCode KSPSolve(KSP k, Vec b, Vec x) {
    Mat A = k->A;
    if (!A || !A->assembled) UNSUPPORTED("KSPSolve without assembled operators");
    if (k->pc == P_MG) return ksp_solve_mg(k, b, x);
    if (k->pc == P_LU) return ksp_solve_direct(k, b, x);            /* exact for preonly / richardson scale 1; damped otherwise */
    if (k->normtype == KSP_NORM_UNPRECONDITIONED) return ksp_solve_monitored(k, b, x);
    if (k->type == K_OTHER) UNSUPPORTED("KSPSolve with a Krylov type other than richardson/chebyshev/preonly");
    if (k->type == K_PREONLY) {                                     /* x = B b: one undamped Richardson step from the zero guess */
        const int g0 = k->guess_nonzero; const PetscInt m0 = k->maxits; const double s0 = k->scale;
        k->type = K_RICHARDSON; k->guess_nonzero = 0; k->maxits = 1; k->scale = 1.0;
        PetscErrorCode rc = KSPSolve(k, b, x);
        k->type = K_PREONLY; k->guess_nonzero = g0; k->maxits = m0; k->scale = s0;
        return rc;
    }
    need_same(b, x, "KSPSolve");
    const int pc = ksp_pc(k);
    const PetscInt maxit = k->maxits;
    if (k->type == K_RICHARDSON && (g_tc_rec || tc_on()) && tc_solve(k, b, x)) return 0;     /* recorded for the tail kernel (above) */
    k->b = b; k->x = x; k->its = 0;
    /* the first sweep was made by the pass that evaluated the last residual norm (norm_of_deferred_residual) and nothing has touched b or x since */
    const int spec = k->spec_ok && k->guess_nonzero && maxit >= k->spec_n && k->type == K_RICHARDSON && k->spec_b == b && k->spec_x == x &&
                     b->ver == k->spec_vb && x->ver == k->spec_vx && k->spec_epoch == g_mat_epoch && !x->lz && !b->lz && !x->host_dirty && !b->host_dirty &&
                     (A->kind == MAT_STENCIL || A->kind == MAT_STENCIL_ROW);
    k->spec_ok = 0;
    if (spec) g_lzstat[8]++;
    /* the adopted sweeps are the whole solve: x and the work vector swap buffers and nothing is written.  A residual b - A x that is still
     * deferred (its norm pass did not store it, norm_of_deferred_residual) then follows the OLD iterate into the work vector instead of being
     * computed now; the reference overwrites it unread (src/solver.c:1534), anything else that reads it, or writes b or the work vector
     * (ksp_work), computes it from there first */
    const int adopt_only = spec && maxit == k->spec_n && k->work[0] && same_layout(k->work[0], x);
    if (adopt_only)
        for (int q = 0; q < g_nlz; q++)
            if (g_lz[q]->lz == LZ_RESIDUAL && g_lz[q]->lz_x == x && g_lz[q] != x && g_lz[q] != k->work[0]) { g_lz[q]->lz_x = k->work[0]; g_lzstat[10]++; }
    /* the right-hand side is R (b_f - A_f u_f), still deferred (MatMult(res) just before, src/solver.c:1535-1536), and the solve starts
     * from the zero guess: restriction and first sweep in one pass */
    struct _p_Mat *rrA = NULL, *rrR = NULL; Vec rrb = NULL, rru = NULL;
    if (b->lz == LZ_RR && !k->guess_nonzero && maxit >= 1 && k->type == K_RICHARDSON && (A->kind == MAT_STENCIL || A->kind == MAT_STENCIL_ROW) &&
        b->lz_A->kind == A->kind && b->padded == 1 && x->padded == 1 && geom_eq(&b->g, &A->gf) && geom_eq(&x->g, &A->gf) && x != b &&
        x != b->lz_b && x != b->lz_x) {
        rrA = b->lz_A; rrR = b->lz_A2; rrb = b->lz_b; rru = b->lz_x;
        (void)vdev(rrb); (void)vdev(rru);
        lz_before_write(b, 1);                               /* consumed below: b_c is written by the fused pass */
        g_lzstat[5]--;
        b->host_dirty = 0;
    }
    (void)vdev(b);
    /* the guess is u + P u_c with the correction still deferred (VecAXPY / MatInterpolateAdd just before, src/solver.c:1540-1542):
     * a Richardson sweep on a stencil operator makes it on the fly (first post-smoothing sweep fused with the prolongation) */
    struct _p_Mat *addP = NULL; Vec addUc = NULL;
    if (x->lz == LZ_ADDP && k->guess_nonzero && maxit >= 1 && k->type == K_RICHARDSON && (A->kind == MAT_STENCIL || A->kind == MAT_STENCIL_ROW) &&
        x->padded == 1 && geom_eq(&x->g, &A->gf) && geom_eq(&x->lz_A->gf, &A->gf) && x->lz_x != b) {
        addP = x->lz_A; addUc = x->lz_x;
        (void)vdev(addUc);
        if (x->host_dirty) vec_upload(x);
        lz_before_write(x, 1);                               /* consumed here: dropped, not computed */
        g_lzstat[1]++; g_lzstat[5]--;
    } else if (!k->guess_nonzero) { lz_before_write(x, 1); (void)vdev(x); }
    else { (void)vdev(x); lz_before_write(x, 0); }
    /* KSPSolve zero-fills x when the guess flag is off; on the stencil path the first sweep overwrites the
     * whole interior without reading x, so the fill is only issued when no sweep follows or on the AIJ path */
    if (!k->guess_nonzero) {
        x->host_dirty = 0;
        /* (the Chebyshev recurrence reads the zero guess as p_{k-1} in its second step) */
        if (maxit <= 0 || k->type == K_CHEBYSHEV || (A->kind != MAT_STENCIL && A->kind != MAT_STENCIL_ROW)) DEV(mgk_memset0(G, x->dev, sizeof(double) * (size_t)x->nalloc, NULL));
    }
    /* (Chebyshev on a stencil operator: the recurrence takes its first step before its loop, max_it = 0 included -- oracle/mgo.c) */
    if (maxit <= 0 && !(k->type == K_CHEBYSHEV && (A->kind == MAT_STENCIL || A->kind == MAT_STENCIL_ROW))) return 0;

    if (A->kind == MAT_STENCIL) {
        need_vec(x, 1, &A->gf, A->n, "KSPSolve");
        const double dinv = (pc == P_JACOBI) ? 1.0 / A->coef[2] : 1.0;
        Vec w = adopt_only ? k->work[0] : ksp_work(k, 0, x);
        if (k->type == K_RICHARDSON) {
            /* sweeps two per pass (temporal blocking) where that beats two launches: 2-D grids of 2047^2 and more
             * (MGPETSC_PAIR_MIN_N overrides the threshold; bit-identical either way) */
            static int pair_min_n = -1;
            if (pair_min_n < 0) { const char *e = getenv("MGPETSC_PAIR_MIN_N"); pair_min_n = e ? atoi(e) : 2047; }
            const int j3 = j3_on() && A->gf.dim == 2 && maxit >= 3;
            for (PetscInt it = 0; it < maxit; it++) {
                if (it == 0 && spec) { if (k->spec_n == 3) it += 2; /* w = J(x) / J(J(J(x))) already */ }
                else if (it == 0 && j3) {
                    /* sweeps 1-3 in one pass; a deferred restriction is made first (without the zero-guess sweep it could emit) */
                    if (rrA) { rr_now(rrA, rrR, rrb, rru, b, NULL, dinv, k->scale, NULL); g_lzstat[7]++; }
                    if (rrA || !k->guess_nonzero) DEV(mgk_jacobi3_2d_zero_f64(G, &A->gf, A->coef, dinv, k->scale, NULL, NULL, b->dev, w->dev, NULL));
                    else if (addP) DEV(mgk_prolong_jacobi3_2d_f64(G, &A->gf, &addP->gc, A->coef, dinv, k->scale, NULL, NULL, b->dev, addUc->dev, x->dev, w->dev, NULL));
                    else DEV(mgk_jacobi3_2d_f64(G, &A->gf, A->coef, dinv, k->scale, NULL, NULL, b->dev, x->dev, w->dev, NULL));
                    it += 2; g_lzstat[14]++;
                }
                else if (it == 0 && rrA) { rr_now(rrA, rrR, rrb, rru, b, w->dev, dinv, k->scale, NULL); g_lzstat[7]++; }
                else if (it == 0 && !k->guess_nonzero) DEV(mgk_jacobi_zero_f64(G, &A->gf, dinv, k->scale, b->dev, w->dev, NULL));
                else if (it == 0 && addP) DEV(mgk_prolong_jacobi_f64(G, &A->gf, &addP->gc, A->coef, dinv, k->scale, b->dev, addUc->dev, x->dev, w->dev, NULL));
                else if (A->gf.dim == 2 && maxit - it >= 2 && A->gf.nx >= pair_min_n) {
                    DEV(mgk_jacobi2_2d_f64(G, &A->gf, A->coef, dinv, k->scale, b->dev, x->dev, w->dev, NULL));
                    it++; g_lzstat[15]++;
                } else DEV(mgk_jacobi_f64(G, &A->gf, A->coef, dinv, k->scale, b->dev, x->dev, w->dev, NULL));
                swap_dev(x, w);
            }
            k->its = maxit;
            return 0;
        }
        /* chebyshev, classic recurrence (see oracle/mgo.c) */
        if (!(k->emax > k->emin && k->emin > 0.0)) UNSUPPORTED("chebyshev without -ksp_chebyshev_eigenvalues emin,emax (no eigenvalue estimation)");
        Vec w2 = ksp_work(k, 1, x);
        double scale = 2.0 / (k->emax + k->emin), alpha = 1.0 - scale * k->emin, Gamma = 1.0;
        double mu = 1.0 / alpha, omegaprod = 2.0 / alpha, ckm1 = 1.0, ck = mu, ckp1;
        double *pkm1 = x->dev, *pk = w->dev, *pkp1 = w2->dev, *t;
        if (!k->guess_nonzero) DEV(mgk_jacobi_zero_f64(G, &A->gf, dinv, scale, b->dev, pk, NULL));
        else DEV(mgk_jacobi_f64(G, &A->gf, A->coef, dinv, scale, b->dev, pkm1, pk, NULL));
        for (PetscInt it = 1; it < maxit; it++) {
            ckp1 = 2.0 * mu * ck - ckm1;
            double omega = omegaprod * ck / ckp1;
            DEV(mgk_cheby_f64(G, &A->gf, A->coef, dinv, 1.0 - omega, omega, omega * Gamma * scale, b->dev, pk, pkm1, pkp1, NULL));
            t = pkm1; pkm1 = pk; pk = pkp1; pkp1 = t;
            ckm1 = ck; ck = ckp1;
        }
        x->dev = pk; w->dev = pkm1; w2->dev = pkp1;
        k->its = maxit > 0 ? maxit : 0;
        return 0;
    }

    if (A->kind == MAT_STENCIL_ROW) {
        need_vec(x, 1, &A->gf, A->n, "KSPSolve");
        mat_device_rowtabs(A);
        const double *dt = (pc == P_JACOBI) ? A->d_dtab : A->d_ones;
        Vec w = adopt_only ? k->work[0] : ksp_work(k, 0, x);
        if (k->type == K_CHEBYSHEV) {                       /* the recurrence of the constant-coefficient branch on the row tables */
            if (!(k->emax > k->emin && k->emin > 0.0)) UNSUPPORTED("chebyshev without -ksp_chebyshev_eigenvalues emin,emax (no eigenvalue estimation)");
            Vec w2 = ksp_work(k, 1, x);
            double scale = 2.0 / (k->emax + k->emin), alpha = 1.0 - scale * k->emin, Gamma = 1.0;
            double mu = 1.0 / alpha, omegaprod = 2.0 / alpha, ckm1 = 1.0, ck = mu, ckp1;
            double *pkm1 = x->dev, *pk = w->dev, *pkp1 = w2->dev, *t;
            if (!k->guess_nonzero) DEV(mgk_jacobi_zero_rowcoef_f64(G, &A->gf, dt, scale, b->dev, pk, NULL));
            else DEV(mgk_rowcoef_f64(G, &A->gf, 0, A->d_ctab, dt, scale, b->dev, pkm1, pk, NULL));
            for (PetscInt it = 1; it < maxit; it++) {
                ckp1 = 2.0 * mu * ck - ckm1;
                double omega = omegaprod * ck / ckp1;
                DEV(mgk_cheby_rowcoef_f64(G, &A->gf, A->d_ctab, dt, 1.0 - omega, omega, omega * Gamma * scale, b->dev, pk, pkm1, pkp1, NULL));
                t = pkm1; pkm1 = pk; pk = pkp1; pkp1 = t;
                ckm1 = ck; ck = ckp1;
            }
            x->dev = pk; w->dev = pkm1; w2->dev = pkp1;
            k->its = maxit > 0 ? maxit : 0;
            return 0;
        }
        const int j3 = j3_on() && A->gf.dim == 2 && maxit >= 3;
        for (PetscInt it = 0; it < maxit; it++) {
            if (it == 0 && spec) { if (k->spec_n == 3) it += 2; /* w = J(x) / J(J(J(x))) already */ }
            else if (it == 0 && j3) {
                if (rrA) { rr_now(rrA, rrR, rrb, rru, b, NULL, 1.0, k->scale, dt); g_lzstat[7]++; }
                if (rrA || !k->guess_nonzero) DEV(mgk_jacobi3_2d_zero_f64(G, &A->gf, NULL, 1.0, k->scale, A->d_ctab, dt, b->dev, w->dev, NULL));
                else if (addP) DEV(mgk_prolong_jacobi3_2d_f64(G, &A->gf, &addP->gc, NULL, 1.0, k->scale, A->d_ctab, dt, b->dev, addUc->dev, x->dev, w->dev, NULL));
                else DEV(mgk_jacobi3_2d_f64(G, &A->gf, NULL, 1.0, k->scale, A->d_ctab, dt, b->dev, x->dev, w->dev, NULL));
                it += 2; g_lzstat[14]++;
            }
            else if (it == 0 && rrA) { rr_now(rrA, rrR, rrb, rru, b, w->dev, 1.0, k->scale, dt); g_lzstat[7]++; }
            else if (it == 0 && !k->guess_nonzero) DEV(mgk_jacobi_zero_rowcoef_f64(G, &A->gf, dt, k->scale, b->dev, w->dev, NULL));
            else if (it == 0 && addP) DEV(mgk_prolong_jacobi_rowcoef_f64(G, &A->gf, &addP->gc, A->d_ctab, dt, k->scale, b->dev, addUc->dev, x->dev, w->dev, NULL));
            else DEV(mgk_rowcoef_f64(G, &A->gf, 0, A->d_ctab, dt, k->scale, b->dev, x->dev, w->dev, NULL));
            swap_dev(x, w);
        }
        k->its = maxit;
        return 0;
    }
    if (A->kind != MAT_GENERIC && A->kind != MAT_LEVELG) UNSUPPORTED("KSPSolve on a transfer operator");
    if (k->type != K_RICHARDSON) UNSUPPORTED("chebyshev on an unrecognised (assembled AIJ) or several-grid level operator");
    if (A->m != A->n) UNSUPPORTED("KSPSolve on a rectangular operator");
    const int blk = (A->kind == MAT_LEVELG);
    if (blk) mat_device_levelg(A); else mat_device_csr(A);
    Vec r = ksp_work(k, 0, x), z = ksp_work(k, 1, x);
    if (!k->guess_nonzero) DEV(mgk_d2d(G, r->dev, b->dev, sizeof(double) * (size_t)b->nalloc, NULL));     /* r = b */
    else if (blk) levelg_apply(A, x, r, -1.0, b, "KSPSolve");
    else csr_apply(A, x, r, -1.0, b, "KSPSolve");                                                          /* r = b - A x */
    for (PetscInt it = 0; it < maxit; it++) {
        if (pc == P_JACOBI) DEV(mgk_flat_pointwise_mult(G, x->nalloc, r->dev, A->d_dinv, z->dev, NULL));   /* z = B r */
        else DEV(mgk_d2d(G, z->dev, r->dev, sizeof(double) * (size_t)r->nalloc, NULL));
        DEV(mgk_flat_axpy(G, x->nalloc, k->scale, z->dev, x->dev, NULL));                                  /* x += s z */
        if (it + 1 < maxit) { if (blk) levelg_apply(A, x, r, -1.0, b, "KSPSolve"); else csr_apply(A, x, r, -1.0, b, "KSPSolve"); }
    }
    k->its = maxit;
    return 0;
}

/* KSPBuildResidual(ksp, NULL, v, &V): V = v = b - A x (src/solver.c:1534,1545) */
PetscErrorCode KSPBuildResidual(KSP k, Vec t, Vec v, Vec *V) {
    (void)t;
    if (!k->b || !k->x) UNSUPPORTED("KSPBuildResidual before KSPSolve");
    if (!v) UNSUPPORTED("KSPBuildResidual with v == NULL");
    MatResidual(k->A, k->b, k->x, v);
    if (v->lz == LZ_RESIDUAL) v->lz_ksp = k;
    if (V) *V = v;
    return 0;
}
/* VecNorm of a residual that KSPBuildResidual deferred (src/solver.c:1545-1546), when the solver that built it is a Richardson smoother
 * with a nonzero guess -- the reference's ksp[0], whose KSPSolve opens the next cycle (:1531) on the same u and b: ONE pass over u and b
 * stores r, reduces sum r^2 and makes that solve's first sweep into the solver's work vector (mgk_jacobi_sumsq_store_f64; 32 B per
 * unknown instead of 24 + 8 + 24).  KSPSolve adopts the sweep if b and u are the same vectors and have not been written since (version
 * counters), otherwise it is ignored; r is a concrete vector afterwards. */
static int norm_of_deferred_residual(Vec r, double *ss) {
    KSP k = r->lz_ksp;
    Mat A = r->lz_A;
    Vec b = r->lz_b, u = r->lz_x;
    if (lazy_on() != 1 || k->A != A || k->type != K_RICHARDSON || !k->guess_nonzero || k->maxits < 1 || k->pc == P_MG || k->pc == P_LU ||
        k->normtype == KSP_NORM_UNPRECONDITIONED || (A->kind != MAT_STENCIL && A->kind != MAT_STENCIL_ROW) || A->gf.dim != 2) return 0;
    if (u == k->work[0] || u == k->work[1] || b == k->work[0] || b == k->work[1]) return 0;      /* (a residual that followed the old iterate into the work vector: the general way) */
    const int pc = ksp_pc(k);
    Vec w = ksp_work(k, 0, u);
    (void)vdev(b); (void)vdev(u);
    const int three = j3_on() && k->maxits >= 3;            /* ... ALL of the next solve's first three sweeps (round 3) */
    /* when those three sweeps ARE the next solve (max_it = 3, the reference's -v 3,3), r need not be stored either: it stays deferred, and
     * the KSPSolve that adopts the sweeps lets it follow the old iterate into the work vector (24 B per unknown instead of 32; the
     * reference overwrites r unread, src/solver.c:1534).  MGPETSC_KEEP_R=0 stores it as before */
    static int keep_r = -1;
    if (keep_r < 0) { const char *e = getenv("MGPETSC_KEEP_R"); keep_r = (e && *e) ? atoi(e) : 1; }
    if (three && k->maxits == 3 && keep_r && r != b && r != u && r != w) {
        if (A->kind == MAT_STENCIL) {
            const double dinv = (pc == P_JACOBI) ? 1.0 / A->coef[2] : 1.0;
            DEV(mgk_jacobi3_2d_sumsq_f64(G, &A->gf, A->coef, dinv, k->scale, NULL, NULL, b->dev, u->dev, w->dev, ss, NULL));
        } else {
            mat_device_rowtabs(A);
            const double *dt = (pc == P_JACOBI) ? A->d_dtab : A->d_ones;
            DEV(mgk_jacobi3_2d_sumsq_f64(G, &A->gf, NULL, 1.0, k->scale, A->d_ctab, dt, b->dev, u->dev, w->dev, ss, NULL));
        }
        k->spec_n = 3;
        k->spec_ok = 1; k->spec_b = b; k->spec_x = u; k->spec_vb = b->ver; k->spec_vx = u->ver; k->spec_epoch = g_mat_epoch;
        g_lzstat[9]++; g_lzstat[14]++;
        return 1;
    }
    lz_before_write(r, 1);                                   /* r is computed by the pass below */
    g_lzstat[5]--;
    r->host_dirty = 0;
    if (A->kind == MAT_STENCIL) {
        const double dinv = (pc == P_JACOBI) ? 1.0 / A->coef[2] : 1.0;
        if (three) DEV(mgk_jacobi3_2d_sumsq_store_f64(G, &A->gf, A->coef, dinv, k->scale, NULL, NULL, b->dev, u->dev, w->dev, r->dev, ss, NULL));
        else DEV(mgk_jacobi_sumsq_store_f64(G, &A->gf, A->coef, dinv, k->scale, NULL, NULL, b->dev, u->dev, w->dev, r->dev, ss, NULL));
    } else {
        mat_device_rowtabs(A);
        const double *dt = (pc == P_JACOBI) ? A->d_dtab : A->d_ones;
        if (three) DEV(mgk_jacobi3_2d_sumsq_store_f64(G, &A->gf, NULL, 1.0, k->scale, A->d_ctab, dt, b->dev, u->dev, w->dev, r->dev, ss, NULL));
        else DEV(mgk_jacobi_sumsq_store_f64(G, &A->gf, NULL, 1.0, k->scale, A->d_ctab, dt, b->dev, u->dev, w->dev, r->dev, ss, NULL));
    }
    k->spec_n = three ? 3 : 1;
    k->spec_ok = 1; k->spec_b = b; k->spec_x = u; k->spec_vb = b->ver; k->spec_vx = u->ver; k->spec_epoch = g_mat_epoch;
    g_lzstat[6]++; if (three) g_lzstat[14]++;
    return 1;
}
PetscErrorCode KSPView(KSP k, PetscViewer viewer) {               /* src/solver.c:1562 */
    (void)viewer;
    static const char *tn[] = {"richardson", "chebyshev", "(unsupported)", "preonly"},
                      *pn[] = {"jacobi (default ILU(0) unavailable)", "jacobi", "none", "mg", "lu (dense inverse applied on the GPU: an exact solve)"};
    printf("KSP Object: 1 MPI process\n  type: %s\n", tn[k->type]);
    if (k->type == K_RICHARDSON) printf("    damping factor=%g\n", k->scale);
    if (k->type == K_CHEBYSHEV) printf("    eigenvalue targets used: min %g, max %g\n", k->emin, k->emax);
    printf("  maximum iterations=%d, %s initial guess\n  using %s norm type for convergence test\n", k->maxits,
           k->guess_nonzero ? "nonzero" : "zero", (k->normtype == KSP_NORM_UNPRECONDITIONED || k->pc == P_MG) ? "UNPRECONDITIONED" : "NONE");
    if (k->pc == P_MG) {
        pcmg *mg = k->pcobj.mg;
        printf("PC Object: 1 MPI process\n  type: mg\n    type is MULTIPLICATIVE, levels=%d cycles=v\n", mg ? mg->levels : 0);
        for (int i = 0; mg && i < mg->levels; i++) {
            printf("  %s level %d -------------------------------\n", i == 0 ? "Coarse grid solver --" : "Down/up solver (pre/post-smoother) on", i);
            KSPView(mg->smooth[i], viewer);
        }
        if (k->A) { printf("  linear system matrix = precond matrix:\n  "); MatView(k->A, viewer); }
        return 0;
    }
    printf("PC Object: 1 MPI process\n  type: %s\n", pn[k->pc]);
    if (k->A) { printf("  linear system matrix = precond matrix:\n  "); MatView(k->A, viewer); }
    printf("  backend: mgpetsc (MI355X / gfx950 HIP kernels, fp64, matrix-free where recognised)\n");
    return 0;
}
PetscErrorCode KSPDestroy(KSP *pk) {
    if (!pk || !*pk) return 0;
    tc_ksp_dying(*pk);
    for (int q = 0; q < g_nlz; q++) if (g_lz[q]->lz_ksp == *pk) g_lz[q]->lz_ksp = NULL;      /* deferred residuals no longer name this solver */
    for (int q = 0; q < 3; q++) if ((*pk)->work[q]) VecDestroy(&(*pk)->work[q]);
    pcmg *mg = (*pk)->pcobj.mg;
    if (mg) {
        for (int i = 0; i < mg->levels; i++) {
            KSPDestroy(&mg->smooth[i]);
            if (mg->own_b[i]) VecDestroy(&mg->b[i]);
            if (mg->own_x[i]) VecDestroy(&mg->x[i]);
            if (mg->own_r[i]) VecDestroy(&mg->r[i]);
        }
        free(mg->smooth); free(mg->interp); free(mg->restr); free(mg->b); free(mg->x); free(mg->r);
        free(mg->own_b); free(mg->own_x); free(mg->own_r); free(mg);
    }
    free(*pk); *pk = NULL;
    return 0;
}
