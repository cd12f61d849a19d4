/* ref_record.c -- RECORDER of what the reference computes on the host before any solve.  Test infrastructure only (oracle/Makefile
 * `_ref/record`, built where the reference tree exists; output only under oracle/_ref/).  It includes the reference's headers, links its
 * UNMODIFIED objects (all but poisson.o) over the drop-in's host build (petsc_shim.c + tests/mock_mgk.cpp) and makes the reference's own calls
 * in the order of src/poisson.c:85-118, without Solve.  The linker's --wrap turns every MatSetValue / VecSetValue of the reference into a line
 * of the output, and MPI_Comm_size / MPI_Comm_rank into the `procs` / `rank` of the command line, so the maps and ranges of any number of
 * ranks are recorded by one process.  With procs > 1 it stops after mapping() (integers and h only).
 *
 *   record npts grids levels map mesh procs rank
 *
 * One record per line, every double as %a:
 *   mesh_h H | coord AXIS N v.. | level L GRIDS NI | gridid L id.. | h L LG h0 h1 | ranges L r.. | global L i j g .. | grid L LG NI NJ idx..
 *   res K NI NJ v.. | pro K NI NJ v.. | call M|V HANDLE ROW COL VALUE MODE (in call order) | handle HANDLE KIND L (KIND 0 A, 1 res, 2 pro, 3 b)
 *   error e0 e1 e2   (GetError, src/solver.c:1211, on u1[i][j] = ((7 i + 3 j) % 11) / 11)
 * tests/golden/make_ref_fixtures.py turns these lines into the committed fixtures. */
#include <stdio.h>
#include <stdlib.h>
#include "header.h"

void GetError(Problem *prob, Mesh *mesh, Array2d u1, double *error);   /* src/solver.c:1211: external linkage, in no header */
PetscErrorCode __real_MatSetValue(Mat A, PetscInt row, PetscInt col, PetscScalar value, InsertMode mode);
PetscErrorCode __real_VecSetValue(Vec v, PetscInt row, PetscScalar value, InsertMode mode);

static int g_procs = 1, g_rank = 0, g_nhandles = 0;
static void *g_handle[256];

static int handle_of(void *p) {
    for (int q = 0; q < g_nhandles; q++) if (g_handle[q] == p) return q;
    if (g_nhandles == 256) { fprintf(stderr, "record: more than 256 handles\n"); exit(3); }
    g_handle[g_nhandles] = p;
    return g_nhandles++;
}

PetscErrorCode __wrap_MatSetValue(Mat A, PetscInt row, PetscInt col, PetscScalar value, InsertMode mode) {
    printf("call M %d %d %d %a %d\n", handle_of(A), row, col, value, (int)mode);
    return __real_MatSetValue(A, row, col, value, mode);
}

PetscErrorCode __wrap_VecSetValue(Vec v, PetscInt row, PetscScalar value, InsertMode mode) {
    printf("call V %d %d 0 %a %d\n", handle_of(v), row, value, (int)mode);
    return __real_VecSetValue(v, row, value, mode);
}

int __wrap_MPI_Comm_size(MPI_Comm comm, int *size) { (void)comm; *size = g_procs; return 0; }
int __wrap_MPI_Comm_rank(MPI_Comm comm, int *rank) { (void)comm; *rank = g_rank; return 0; }

static void ints(const char *tag, int a, int b, const int *v, int n) {
    printf("%s %d", tag, a);
    if (b >= 0) printf(" %d", b);
    for (int q = 0; q < n; q++) printf(" %d", v[q]);
    printf("\n");
}

static void stencil(const char *tag, int k, const Array2d *a) {
    printf("%s %d %d %d", tag, k, a->ni, a->nj);
    for (int q = 0; q < a->ni * a->nj; q++) printf(" %a", a->data[q]);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 8) { fprintf(stderr, "usage: record npts grids levels map mesh procs rank\n"); return 1; }
    const int npts = atoi(argv[1]), map = atoi(argv[4]), meshflag = atoi(argv[5]);
    Problem prob;
    Mesh mesh;
    Indices indices;
    Operator op;
    Solver solver;
    g_procs = atoi(argv[6]); g_rank = atoi(argv[7]);
    if (npts < 5 || meshflag < 0 || meshflag > 2 || map < 0 || map > 2 || g_procs < 1 || g_rank < 0 || g_rank >= g_procs) return 1;
    indices.totalGrids = atoi(argv[2]); indices.levels = atoi(argv[3]);
    PetscInitialize(NULL, NULL, NULL, NULL);
    SetUpProblem(&prob);
    for (int i = 0; i < DIMENSION; i++) { mesh.n[i] = npts; mesh.bounds[2 * i] = 0.0; mesh.bounds[2 * i + 1] = 1.0; }
    SetUpMesh(&mesh, meshflag == 0 ? UNIFORM : meshflag == 1 ? NONUNIFORM1 : NONUNIFORM2);
    printf("mesh_h %a\n", mesh.h);
    for (int a = 0; a < DIMENSION; a++) {
        printf("coord %d %d", a, mesh.n[a]);
        for (int j = 0; j < mesh.n[a]; j++) printf(" %a", mesh.coord[a][j]);
        printf("\n");
    }
    indices.coarseningFactor = 2;
    SetUpIndices(&mesh, &indices);
    mapping(&indices, map);
    for (int l = 0; l < indices.levels; l++) {
        const Level *L = &indices.level[l];
        printf("level %d %d %d\n", l, L->grids, L->global.ni);
        ints("gridid", l, -1, L->gridId, L->grids);
        for (int lg = 0; lg < L->grids; lg++) printf("h %d %d %a %a\n", l, lg, L->h[lg][0], L->h[lg][1]);
        ints("ranges", l, -1, L->ranges, g_procs + 1);
        ints("global", l, -1, L->global.data, L->global.ni * L->global.nj);
        for (int lg = 0; lg < L->grids; lg++) {
            printf("grid %d %d %d %d", l, lg, L->grid[lg].ni, L->grid[lg].nj);
            for (int q = 0; q < L->grid[lg].ni * L->grid[lg].nj; q++) printf(" %d", L->grid[lg].data[q]);
            printf("\n");
        }
    }
    if (g_procs > 1) return 0;
    SetUpOperator(&indices, &op);
    GridTransferOperators(op, indices);
    for (int k = 0; k < op.totalGrids - 1; k++) { stencil("res", k, &op.res[k]); stencil("pro", k, &op.pro[k]); }
    solver.numIter = 1; solver.moreInfo = 0; solver.v[0] = solver.v[1] = 1;
    SetUpSolver(&indices, &solver, VCYCLE);
    Assemble(&prob, &mesh, &indices, &op, &solver);
    const Assembly *as = solver.assem;
    for (int l = 0; l < as->levels; l++) printf("handle %d 0 %d\n", handle_of(as->A[l]), l);
    /* the transfers exist where every level above the last holds one grid (src/solver.c:1042-1047): the stream shows whether they were filled */
    for (int q = 0; q < g_nhandles; q++)
        for (int l = 0; l < as->levels - 1; l++) {
            if (g_handle[q] == (void *)as->res[l]) printf("handle %d 1 %d\n", q, l);
            if (g_handle[q] == (void *)as->pro[l]) printf("handle %d 2 %d\n", q, l);
        }
    printf("handle %d 3 0\n", handle_of(as->b[0]));
    Array2d u1;
    double err[3];
    CreateArray2d(npts - 2, npts - 2, &u1);
    for (int i = 0; i < u1.ni; i++) for (int j = 0; j < u1.nj; j++) u1.data[i * u1.nj + j] = ((7 * i + 3 * j) % 11) / 11.0;
    GetError(&prob, &mesh, u1, err);
    printf("error %a %a %a\n", err[0], err[1], err[2]);
    return 0;
}
