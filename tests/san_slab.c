/* tests/san_slab.c -- TEST INFRASTRUCTURE: the slab (multi-rank) host logic of csrc/mg_solver.c + csrc/mg_comm.c under
 * AddressSanitizer / UBSan on the CPU, over tests/mock_mgk.cpp.  P loopback ranks (threads) solve the 3-D problem; the
 * concatenated solution must equal the single-rank one bit for bit; the transport self-test runs on every rank, and the
 * phantom communicator drives one rank of 8 through a few cycles.  usage: san_slab P npts levels dist_min_n [mixed]
 * san_slab P npts levels dist_min_n rhs|rhs_mixed b1.bin b2.bin out_prefix: right-hand sides from the caller (whole fine grids of doubles written by the
 * test).  Every rank hands mg_solver_set_rhs_host its own planes of b1, solves, then loads its planes of b2 into the SAME solver and solves again;
 * both results must equal the single rank's, and the second one a fresh solver's on b2 -- iterations, ||b||, history and field bit for bit.  The
 * single rank's fields and histories go to out_prefix{1,2}.{u,rn} for the test to compare with the oracle. */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mgsolve.h"
#include "mg_comm.h"

typedef struct { pthread_barrier_t bar; char blobs[MGK_PEER_MAX][MG_PEER_BLOB_BYTES]; } peer_boot;      /* the launcher's all-gather of the handle blobs */
typedef struct { int rank, P, npts, levels, dmin, mixed, rc; void *shared; double *u; long n; int it; peer_boot *boot;
                 const double *b[2]; int nb; double *ub[2]; int itb[2]; double bn[2]; double rn[2][64]; } job;

static void cfg(mg_config *c, const job *j, int rank, int P) {
    mg_config_default(c);
    c->dim = 3; c->npts = j->npts; c->levels = j->levels; c->scale = 6.0 / 7.0; c->maxiter = 60;
    c->rank = rank; c->nranks = P; c->dist_min_n = j->dmin; c->precision = j->mixed ? MG_PREC_MIXED : MG_PREC_FP64;
    c->pair_min_n = 7;                /* two-sweep passes on the small test levels too */
}
static void *work(void *p) {
    job *j = (job *)p;
    mg_comm *cm = NULL;
    if (j->P > 1 && j->boot) {
        /* the peer transport (mailboxes + flag words): planes of the finest level, 5 fields per exchange, gather box for the whole 3-D level */
        mgk_geom g0; mgk_geom_init(&g0, 3, j->npts - 2, j->npts - 2, j->npts - 2);
        cm = mg_comm_peer_create(j->rank, j->P, 0, sizeof(double) * (size_t)g0.plane, 5, sizeof(double) * (size_t)g0.total, j->boot->blobs[j->rank]);
        pthread_barrier_wait(&j->boot->bar);
        if (!cm || mg_comm_peer_connect(cm, j->boot->blobs)) { fprintf(stderr, "peer: %s\n", mg_comm_last_error()); return NULL; }
        pthread_barrier_wait(&j->boot->bar);
    } else if (j->P > 1) cm = mg_comm_loopback_create(j->shared, j->rank);
    mg_config c; cfg(&c, j, j->rank, j->P);
    mg_solver *s = NULL;
    j->rc = 1;
    if (j->P > 1) {
        mgk_ctx *ctx = NULL;
        if (mgk_ctx_create(&ctx, 0) || mg_comm_selftest(cm, ctx)) { fprintf(stderr, "selftest: %s\n", mg_comm_last_error()); return NULL; }
        mgk_ctx_destroy(ctx);
    }
    if (mg_solver_create(&s, &c, cm)) { fprintf(stderr, "create: %s\n", mg_last_error()); return NULL; }
    if (mg_solver_set_rhs_problem(s) || mg_solver_solve(s)) { fprintf(stderr, "solve: %s\n", mg_last_error()); return NULL; }
    j->n = mg_solver_local_unknowns(s);
    j->u = (double *)malloc(sizeof(double) * (size_t)j->n);
    j->it = mg_solver_iterations(s);
    double e[3];
    if (mg_solver_get_solution(s, j->u) || mg_solver_error_norms(s, e)) { fprintf(stderr, "fetch: %s\n", mg_last_error()); return NULL; }
    /* fixed-count cycling with deferred norms as bench.py does it */
    if (mg_solver_reset(s) || mg_solver_cycles(s, 3) || mg_solver_sync(s)) { fprintf(stderr, "cycles: %s\n", mg_last_error()); return NULL; }
    mg_solver_destroy(s);
    if (cm) mg_comm_destroy(cm);
    j->rc = 0;
    return NULL;
}

/* right-hand sides from the caller: j->b[0 .. nb-1] one after the other on one solver object */
static void *rhs_work(void *p) {
    job *j = (job *)p;
    mg_comm *cm = j->P > 1 ? mg_comm_loopback_create(j->shared, j->rank) : NULL;
    mg_config c; cfg(&c, j, j->rank, j->P);
    mg_solver *s = NULL;
    j->rc = 1;
    if (mg_solver_create(&s, &c, cm)) { fprintf(stderr, "create: %s\n", mg_last_error()); return NULL; }
    int z0 = 0;
    const int nz = mg_solver_level_local_planes(s, 0, &z0);
    const long n = j->npts - 2, plane = n * n;
    j->n = mg_solver_local_unknowns(s);
    if (j->n != plane * nz) { fprintf(stderr, "rank %d: %ld local unknowns, %d planes\n", j->rank, j->n, nz); return NULL; }
    for (int q = 0; q < j->nb; q++) {
        if (mg_solver_set_rhs_host(s, j->b[q] + plane * z0) || mg_solver_solve(s)) { fprintf(stderr, "solve: %s\n", mg_last_error()); return NULL; }
        j->ub[q] = (double *)malloc(sizeof(double) * (size_t)j->n);
        j->itb[q] = mg_solver_iterations(s);
        j->bn[q] = mg_solver_bnorm(s);
        if (j->itb[q] >= 64) { fprintf(stderr, "history too long\n"); return NULL; }
        memcpy(j->rn[q], mg_solver_rnorm(s), sizeof(double) * (size_t)(j->itb[q] + 1));
        if (mg_solver_get_solution(s, j->ub[q])) { fprintf(stderr, "fetch: %s\n", mg_last_error()); return NULL; }
    }
    mg_solver_destroy(s);
    if (cm) mg_comm_destroy(cm);
    j->rc = 0;
    return NULL;
}
static double *read_field(const char *path, long n) {
    FILE *f = fopen(path, "rb");
    double *b = (double *)malloc(sizeof(double) * (size_t)n);
    if (!f || !b || fread(b, sizeof(double), (size_t)n, f) != (size_t)n) { fprintf(stderr, "cannot read %ld doubles from %s\n", n, path); exit(2); }
    fclose(f);
    return b;
}
static int write_doubles(const char *prefix, int q, const char *ext, const double *x, long n) {
    char path[1024];
    snprintf(path, sizeof(path), "%s%d.%s", prefix, q + 1, ext);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(x, sizeof(double), (size_t)n, f) != (size_t)n) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    return fclose(f);
}
static int run_ranks(job *js, const job *base, int P, const double *b0, const double *b1) {
    pthread_t *th = (pthread_t *)calloc((size_t)P, sizeof(pthread_t));
    void *shared = P > 1 ? mg_comm_loopback_shared_create(P) : NULL;
    for (int r = 0; r < P; r++) {
        js[r] = *base; js[r].rank = r; js[r].P = P; js[r].shared = shared; js[r].b[0] = b0; js[r].b[1] = b1; js[r].nb = b1 ? 2 : 1;
        pthread_create(&th[r], NULL, rhs_work, &js[r]);
    }
    int bad = 0;
    for (int r = 0; r < P; r++) { pthread_join(th[r], NULL); bad |= js[r].rc; }
    if (shared) mg_comm_loopback_shared_destroy(shared);
    free(th);
    return bad;
}
/* ranks js[0 .. P-1], right-hand side qa of theirs, against the single job `one`, right-hand side qb of its: everything bit for bit but the norms of
 * several ranks, which are sums in another order (1e-13, the bar of the slab tests) */
static int same_as(const job *js, int P, int qa, const job *one, int qb, const char *what) {
    long off = 0; int bad = 0;
    for (int r = 0; r < P; r++) {
        const job *j = &js[r];
        if (j->itb[qa] != one->itb[qb]) { fprintf(stderr, "%s: rank %d made %d cycles, %d expected\n", what, r, j->itb[qa], one->itb[qb]); return 1; }
        for (int k = 0; k <= j->itb[qa]; k++) {
            const double a = j->rn[qa][k], b = one->rn[qb][k];
            if (P == 1 ? a != b : fabs(a - b) > 1e-13 * b) { fprintf(stderr, "%s: rank %d, norm %d: %.17g vs %.17g\n", what, r, k, a, b); bad = 1; }
        }
        if (P == 1 ? j->bn[qa] != one->bn[qb] : fabs(j->bn[qa] - one->bn[qb]) > 1e-13 * one->bn[qb]) { fprintf(stderr, "%s: rank %d: ||b||\n", what, r); bad = 1; }
        if (off + j->n > one->n || memcmp(j->ub[qa], one->ub[qb] + off, sizeof(double) * (size_t)j->n)) { fprintf(stderr, "%s: rank %d: the field differs\n", what, r); bad = 1; }
        off += j->n;
    }
    if (off != one->n) { fprintf(stderr, "%s: slabs do not add up\n", what); bad = 1; }
    return bad;
}
static int rhs_run(int P, const job *base, const char *f1, const char *f2, const char *prefix) {
    const long n = base->npts - 2, N = n * n * n;
    double *b1 = read_field(f1, N), *b2 = read_field(f2, N);
    job one, fresh1, *js = (job *)calloc((size_t)P, sizeof(job)), *fr = (job *)calloc((size_t)P, sizeof(job));
    int bad = run_ranks(&one, base, 1, b1, b2) || run_ranks(&fresh1, base, 1, b2, NULL) || run_ranks(js, base, P, b1, b2) || run_ranks(fr, base, P, b2, NULL);
    if (bad) { fprintf(stderr, "a run failed\n"); return 1; }
    bad |= same_as(&one, 1, 1, &fresh1, 0, "one rank, live solver against a fresh one");
    bad |= same_as(js, P, 0, &one, 0, "ranks against one rank, first right-hand side");
    bad |= same_as(js, P, 1, &one, 1, "ranks against one rank, second right-hand side");
    for (int r = 0; r < P; r++) {               /* rank by rank: the same reduction order, so the norms are the same bits too */
        const job *a = &js[r], *f = &fr[r];
        if (a->itb[1] != f->itb[0] || a->bn[1] != f->bn[0] || memcmp(a->rn[1], f->rn[0], sizeof(double) * (size_t)(f->itb[0] + 1)) ||
            memcmp(a->ub[1], f->ub[0], sizeof(double) * (size_t)f->n)) { fprintf(stderr, "rank %d: the live solver differs from a fresh one on the second right-hand side\n", r); bad = 1; }
    }
    for (int q = 0; q < 2; q++) bad |= write_doubles(prefix, q, "u", one.ub[q], N) || write_doubles(prefix, q, "rn", one.rn[q], one.itb[q] + 1);
    for (int r = 0; r < P; r++) { free(js[r].ub[0]); free(js[r].ub[1]); free(fr[r].ub[0]); }
    free(one.ub[0]); free(one.ub[1]); free(fresh1.ub[0]); free(js); free(fr); free(b1); free(b2);
    printf("SAN_SLAB_RHS_%s P=%d cycles=%d,%d\n", bad ? "FAILED" : "OK", P, one.itb[0], one.itb[1]);
    return bad;
}

/* the first-run gate with a transport that delivers ONE wrong plane (rank `bad` gets a wrong lo ghost): every rank must come back
 * from mg_comm_selftest -- nobody left inside a collective --, the rank that saw the wrong plane with MGK_ECOMM and its message,
 * the others with 0 */
typedef struct { int rank; void *shared; int rc; char msg[512]; } fjob;
static void *fault_work(void *p) {
    fjob *j = (fjob *)p;
    mg_comm *cm = mg_comm_loopback_create(j->shared, j->rank);
    mgk_ctx *ctx = NULL;
    j->rc = -1;
    if (!cm || mgk_ctx_create(&ctx, 0)) return NULL;
    j->rc = mg_comm_selftest(cm, ctx);
    snprintf(j->msg, sizeof(j->msg), "%s", mg_comm_last_error());
    mgk_ctx_destroy(ctx);
    mg_comm_destroy(cm);
    return NULL;
}
static int fault_run(int P, int bad_rank) {
    fjob *js = (fjob *)calloc((size_t)P, sizeof(fjob));
    pthread_t *th = (pthread_t *)calloc((size_t)P, sizeof(pthread_t));
    void *shared = mg_comm_loopback_shared_create(P);
    mg_comm_loopback_inject_fault(shared, bad_rank);
    for (int r = 0; r < P; r++) { js[r].rank = r; js[r].shared = shared; pthread_create(&th[r], NULL, fault_work, &js[r]); }
    int bad = 0;
    for (int r = 0; r < P; r++) {
        pthread_join(th[r], NULL);
        const int want = (r == bad_rank) ? MGK_ECOMM : 0;
        if (js[r].rc != want) { fprintf(stderr, "fault run: rank %d returned %d (%s), expected %d\n", r, js[r].rc, js[r].msg, want); bad = 1; }
        if (r == bad_rank && !strstr(js[r].msg, "halo plane")) { fprintf(stderr, "fault run: rank %d does not name the first mismatch: %s\n", r, js[r].msg); bad = 1; }
    }
    mg_comm_loopback_shared_destroy(shared);
    free(js); free(th);
    printf("SAN_FAULT_%s P=%d bad_rank=%d\n", bad ? "FAILED" : "OK", P, bad_rank);
    return bad;
}

/* the peer transport when a neighbour never shows up: rank 0 of 2 exchanges a halo and all-reduces; rank 1 maps the memory and then does
 * nothing.  With MG_PEER_TIMEOUT_S = 1 rank 0 must come back from both calls within seconds and the all-reduce (a host-synchronising hook)
 * must report MGK_ECOMM -- never a hang */
static void *timeout_work(void *p) {
    job *j = (job *)p;
    mgk_geom g; mgk_geom_init(&g, 3, 15, 7, 3);
    mg_comm *cm = mg_comm_peer_create(j->rank, 2, 0, sizeof(double) * (size_t)g.plane, 2, sizeof(double) * (size_t)g.total, j->boot->blobs[j->rank]);
    pthread_barrier_wait(&j->boot->bar);
    j->rc = -1;
    if (!cm || mg_comm_peer_connect(cm, j->boot->blobs)) return NULL;
    pthread_barrier_wait(&j->boot->bar);
    if (j->rank == 0) {
        mgk_ctx *ctx = NULL;
        void *f = NULL;
        double v = 1.0;
        if (mgk_ctx_create(&ctx, 0) || mgk_malloc(ctx, &f, sizeof(double) * (size_t)g.total)) return NULL;
        int r1 = cm->halo(cm, ctx, f, &g, 8, mgk_stream_comm(ctx));
        int r2 = cm->allreduce_sum(cm, ctx, &v, 1, NULL);
        j->rc = (r1 == 0 && r2 == MGK_ECOMM && cm->check(cm) == MGK_ECOMM) ? 0 : 100 + r2;
        mgk_free(ctx, f);
        mgk_ctx_destroy(ctx);
    } else j->rc = 0;
    pthread_barrier_wait(&j->boot->bar);                      /* rank 1 keeps its memory mapped until rank 0 is through */
    mg_comm_destroy(cm);
    return NULL;
}
static int timeout_run(void) {
    setenv("MG_PEER_TIMEOUT_S", "1", 1);
    peer_boot *boot = (peer_boot *)calloc(1, sizeof(peer_boot));
    pthread_barrier_init(&boot->bar, NULL, 2);
    job js[2]; memset(js, 0, sizeof(js));
    pthread_t th[2];
    for (int r = 0; r < 2; r++) { js[r].rank = r; js[r].boot = boot; pthread_create(&th[r], NULL, timeout_work, &js[r]); }
    for (int r = 0; r < 2; r++) pthread_join(th[r], NULL);
    const int bad = js[0].rc || js[1].rc;
    if (bad) fprintf(stderr, "timeout run: rank 0 rc %d, rank 1 rc %d (%s)\n", js[0].rc, js[1].rc, mg_comm_last_error());
    pthread_barrier_destroy(&boot->bar); free(boot);
    printf("SAN_PEER_TIMEOUT_%s\n", bad ? "FAILED" : "OK");
    return bad;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "peer_timeout")) return timeout_run();
    if (argc == 4 && !strcmp(argv[1], "fault")) return fault_run(atoi(argv[2]), atoi(argv[3]));
    if (argc < 5) { fprintf(stderr, "usage: san_slab P npts levels dist_min_n [mixed|peer] | san_slab fault P bad_rank\n"); return 2; }
    const int P = atoi(argv[1]);
    job base; memset(&base, 0, sizeof(base));
    base.npts = atoi(argv[2]); base.levels = atoi(argv[3]); base.dmin = atoi(argv[4]); base.mixed = argc > 5 && !strcmp(argv[5], "mixed");
    if (argc == 9 && !strncmp(argv[5], "rhs", 3)) { base.mixed = !strcmp(argv[5], "rhs_mixed"); return rhs_run(P, &base, argv[6], argv[7], argv[8]); }
    const int use_peer = argc > 5 && !strcmp(argv[5], "peer");        /* the ranks talk through the peer transport instead of loopback */
    job one = base; one.P = 1;
    work(&one);
    if (one.rc) return 1;
    job *js = (job *)calloc((size_t)P, sizeof(job));
    pthread_t *th = (pthread_t *)calloc((size_t)P, sizeof(pthread_t));
    void *shared = mg_comm_loopback_shared_create(P);
    peer_boot *boot = NULL;
    if (use_peer) { boot = (peer_boot *)calloc(1, sizeof(peer_boot)); pthread_barrier_init(&boot->bar, NULL, (unsigned)P); }
    for (int r = 0; r < P; r++) { js[r] = base; js[r].rank = r; js[r].P = P; js[r].shared = shared; js[r].boot = boot; pthread_create(&th[r], NULL, work, &js[r]); }
    long off = 0; int bad = 0;
    for (int r = 0; r < P; r++) {
        pthread_join(th[r], NULL);
        if (js[r].rc || js[r].it != one.it) { fprintf(stderr, "rank %d failed (rc %d, %d vs %d cycles)\n", r, js[r].rc, js[r].it, one.it); bad = 1; continue; }
        if (off + js[r].n > one.n || memcmp(js[r].u, one.u + off, sizeof(double) * (size_t)js[r].n)) { fprintf(stderr, "rank %d: solution differs from the single-rank one\n", r); bad = 1; }
        off += js[r].n;
        free(js[r].u);
    }
    if (off != one.n) { fprintf(stderr, "slabs do not add up\n"); bad = 1; }
    mg_comm_loopback_shared_destroy(shared);
    /* one rank of 8 on the phantom communicator (timing aid): the code path only */
    mg_comm *ph = mg_comm_phantom_create(3, 8, 1.0, 50.0);
    mg_config c; job pj = base; pj.dmin = base.dmin; cfg(&c, &pj, 3, 8);
    mg_solver *s = NULL;
    if (!ph || mg_solver_create(&s, &c, ph) || mg_solver_set_rhs_problem(s) || mg_solver_cycles(s, 2) || mg_solver_sync(s)) { fprintf(stderr, "phantom: %s\n", mg_last_error()); bad = 1; }
    if (s) mg_solver_destroy(s);
    if (ph) mg_comm_destroy(ph);
    free(one.u); free(js); free(th);
    if (boot) { pthread_barrier_destroy(&boot->bar); free(boot); }
    printf("SAN_SLAB_%s P=%d cycles=%d%s\n", bad ? "FAILED" : "OK", P, one.it, use_peer ? " transport=peer" : "");
    return bad;
}
