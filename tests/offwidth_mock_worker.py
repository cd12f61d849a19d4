"""Worker of tests/test_offwidth_cycle_cpu.py: the cases of tests/offwidth_cases.py with the product's Solver over csrc/mg_solver.c + mg_comm.c +
tests/mock_mgk.cpp (the library of tools/stress_solver_mock.py, injected into the package's loader here: a process of its own, because the loader
caches the libraries it hands out).  argv: the sizes of the 3-D cases, the sizes of the 2-D cases, the size of the slab case (comma lists).  Prints
one line per case and `offwidth mock: N cases, 0 mismatches`; an assertion ends it with a traceback."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    from stress_solver_mock import inject
    inject()
    import offwidth_cases as OW
    from multigrid_petsc_amd.comm import LoopbackWorld
    from multigrid_petsc_amd.solver import Solver
    from oracle import Oracle
    orc = Oracle()
    sizes3, sizes2, slab = ([int(x) for x in a.split(",") if x] for a in sys.argv[1:4])
    n = 0
    for npts in sizes3:
        for precision in ("fp64", "mixed"):
            for kw in OW.VARIANTS_3D:
                OW.check3d(Solver, orc, npts, precision, kw)
                n += 1
                print(f"ok 3-D {npts} {precision} {kw}", flush=True)
    for npts in sizes2:
        for mesh in (0, 1, 2):
            for cheby in (False, True):
                OW.check2d(Solver, orc, npts, mesh, cheby, 5, {})
                n += 1
                print(f"ok 2-D {npts} mesh {mesh} {'chebyshev' if cheby else 'richardson'}: five cycles", flush=True)
        for kw in ({}, {"fuse": 0}, {"pair_min_n": 7}):
            OW.check2d(Solver, orc, npts, 0, False, 0, kw)
            n += 1
            print(f"ok 2-D {npts} uniform mesh, solved {kw}", flush=True)

    def solve_ranks(P, npts, levels, scale, maxiter, dist_min_n, **kw):
        world = LoopbackWorld(P)

        def fn(rank, comm):
            s = Solver(3, npts, levels, scale=scale, maxiter=maxiter, rank=rank, nranks=P, comm=comm, dist_min_n=dist_min_n, **kw)
            s.set_rhs_problem()
            it = s.solve()
            res = (it, s.rnorm, s.solution(), s.error_norms(), [s.level_planes(l) for l in range(levels)])
            s.close()
            return res
        try:
            return world.run(fn)
        finally:
            world.close()
    for npts in slab:
        for P in (2, 3):
            OW.check_slabs(solve_ranks, orc, P, npts, dist_min_n=11)
            n += 1
            print(f"ok {P} slab ranks at {npts}", flush=True)
    # a depth whose coarsest width would be even (25: 23, 11, 5, 2) is refused, and the message states the condition that is checked
    from multigrid_petsc_amd.solver import MgError
    for dim, npts, levels in ((3, 25, 4), (2, 97, 6), (2, 1000, 3)):
        try:
            Solver(dim, npts, levels)
            raise SystemExit(f"Solver({dim}, {npts}, {levels}) was accepted")
        except MgError as e:
            assert "divisible by 2^(levels-1)" in str(e) and "odd" in str(e) and "2^m" not in str(e), str(e)
    print(f"offwidth mock: {n} cases, 0 mismatches")


if __name__ == "__main__":
    main()
