"""Worker of tests/test_xline_cpu.py: the product's Solver over a shared library that holds mg_solver.c, mg_comm.c, mg_line.c, mg_xline.c and
the host-memory stand-ins (tests/mock_mgk_xline.cpp) in place of libmgk.so / libmgpetsc.so.  A process of its own, because the loader caches
the libraries it hands out.  argv: library, output .npz, then one 'pc,npts,levels,mesh,rhs' per case (rhs: 'manufactured' or 'rough:<seed>',
tests/rhs_cases.uniform).  Every case: Solver(pc_type=pc, scale=0.8) with the defaults (and the log of line passes), reset + solve, graph=0,
fuse=0 ("--without-mg-xline" instead of the cases: only what a library linked without mg_xline.c must do).  Then v = (2, 1) and v = (3, 3) logs on a small case, yline and jacobi solves on this build, the x tables of mg_xline.c, the
refusals."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
SCALE = 0.8
TABLE_LEVELS = [(17, 0, 0), (17, 3, 0), (17, 1, 1), (17, 3, 1), (33, 0, 2), (33, 4, 2), (65, 0, 1)]     # (npts, level, mesh); level 3 of 17 / 4 of 33: n = 1


def main():
    so, out = sys.argv[1], sys.argv[2]
    import multigrid_petsc_amd._lib as loader
    lib = ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)
    loader._cache["mgk"] = lib
    loader._cache["mgpetsc"] = lib
    import rhs_cases
    from multigrid_petsc_amd.solver import MgError, Solver
    if sys.argv[3:] == ["--without-mg-xline"]:
        # a library linked without mg_xline.c (the y-line tier's link): the new smoothers are refused with a message, yline still runs
        for pc in ("xline", "altline"):
            try:
                Solver(2, 17, 4, scale=SCALE, pc_type=pc)
                raise SystemExit(f"{pc} was accepted")
            except MgError as e:
                assert "mg_xline.c is not linked" in str(e), str(e)
        s = Solver(2, 17, 4, maxiter=100, scale=SCALE, mesh=1, pc_type="yline")
        s.set_rhs_problem()
        np.savez(out, it=s.solve(), u=s.solution())
        s.close()
        return
    lib.mock_xline_log.restype = ctypes.c_char_p
    res = {}

    def make(pc, npts, levels, mesh, rhs, v=(3, 3), **kw):
        s = Solver(2, npts, levels, v=v, maxiter=100, scale=SCALE, mesh=mesh, pc_type=pc, **kw)
        if rhs == "manufactured":
            s.set_rhs_problem()
        else:
            s.set_rhs(rhs_cases.uniform(2, npts, int(rhs.split(":")[1])))
        return s

    for case in sys.argv[3:]:
        f = case.split(",")
        pc, npts, levels, mesh, rhs = f[0], int(f[1]), int(f[2]), int(f[3]), f[4]
        k = case + ":"
        s = make(pc, npts, levels, mesh, rhs)
        lib.mock_xline_log_clear()
        it = s.solve()
        res[k + "it"], res[k + "rn"], res[k + "u"], res[k + "bnorm"] = it, s.rnorm, s.solution(), s.bnorm
        res[k + "log"] = lib.mock_xline_log().decode()
        res[k + "dof"] = s.dof_updates_per_cycle
        s.reset()
        assert s.solve() == it and np.array_equal(s.rnorm, res[k + "rn"]) and np.array_equal(s.solution(), res[k + "u"]), "reset + solve differs"
        s.close()
        for tag, kw in (("graph0", dict(graph=0)), ("fuse0", dict(fuse=0))):
            s = make(pc, npts, levels, mesh, rhs, **kw)
            res[k + tag + "_it"], res[k + tag + "_rn"], res[k + tag + "_u"] = s.solve(), s.rnorm, s.solution()
            s.close()
    # the order of the passes under other sweep counts (17, 4 levels, mesh 1; the coarse levels run inside the recorded graph or not)
    for v in ((2, 1), (3, 3), (1, 2)):
        for graph in (1, 0):
            s = make("altline", 17, 4, 1, "manufactured", v=v, graph=graph)
            lib.mock_xline_log_clear()
            it = s.solve()
            k = f"order:{v[0]},{v[1]},{graph}:"
            res[k + "it"], res[k + "log"], res[k + "u"], res[k + "rn"] = it, lib.mock_xline_log().decode(), s.solution(), s.rnorm
            s.close()
    # pc_type 0 and 1 on this build
    for pc, npts, levels, mesh in (("yline", 65, 6, 1), ("yline", 17, 4, 2), ("jacobi", 33, 5, 0), ("jacobi", 33, 5, 1)):
        s = make(pc, npts, levels, mesh, "manufactured")
        k = f"old:{pc},{npts},{levels},{mesh}:"
        res[k + "it"], res[k + "rn"], res[k + "u"] = s.solve(), s.rnorm, s.solution()
        s.close()
    # the x table of mg_xline.c from the oracle's rows (the caller passes them as files: this process does not load the oracle)
    lib.mg_xline_stride.restype = ctypes.c_long
    lib.mg_xline_stride.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.mg_xline_factor.restype = None
    lib.mg_xline_factor.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    rows = np.load(out + ".rows.npz")
    for npts, level, mesh in TABLE_LEVELS:
        k = f"tab:{npts},{level},{mesh}"
        ct = np.ascontiguousarray(rows[k])
        n = ct.shape[0]
        gs = lib.mg_xline_stride(n, int(mesh == 0))
        assert (gs == 0) if mesh == 0 else (gs >= n and gs % 16 == 0), gs
        nrows = 1 if mesh == 0 else n
        g = np.full(n if mesh == 0 else n * gs, 0.0)
        lib.mg_xline_factor(n, nrows, ct.ctypes.data_as(ctypes.c_void_p), gs, g.ctypes.data_as(ctypes.c_void_p))
        res[k] = g[:n].reshape(1, n) if mesh == 0 else g.reshape(n, gs)
    # what the line smoothers are not built for is refused at creation, with the reason and under their own name
    for pc, name in (("xline", "x-line"), ("altline", "alternating line")):
        for kw, msg in ((dict(dim=3, npts=17, levels=3), "built for 2-D"),
                        (dict(dim=2, npts=17, levels=3, precision="mixed"), "not mixed precision"),
                        (dict(dim=2, npts=17, levels=3, ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev"),
                        (dict(dim=2, npts=17, levels=3, nranks=2), "one GPU")):
            try:
                Solver(v=(3, 3), maxiter=20, scale=SCALE, pc_type=pc, **kw)
                raise SystemExit(f"{pc} {kw} was accepted")
            except MgError as e:
                assert msg in str(e) and name in str(e), str(e)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
