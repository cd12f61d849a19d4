"""Worker of tests/test_xchunkline_cpu.py: the product's Solver over a shared library that holds mg_solver.c, mg_comm.c, mg_line.c, mg_xline.c,
mg_line_chunk.c, mg_xline_chunk.c and the host-memory stand-ins (tests/mock_mgk_xchunkline.cpp) in place of libmgk.so / libmgpetsc.so.  A
process of its own, because the loader caches the libraries it hands out.  argv: library, output .npz, then one
'pc;xc;yc;npts,levels,mesh,rhs' per case (rhs: 'manufactured' or 'rough:<seed>', tests/rhs_cases.uniform).  Every case:
Solver(pc_type=pc, xline_chunk=xc, line_chunk=yc, scale=0.8) with the defaults (and the execution counts of the stand-ins: plain y forward /
backward, plain x forward / backward, the four chunked y passes, the four chunked x passes), reset + solve, graph=0, fuse=0.  xc = 0 runs
once more without the keyword.  With '--unlinked' as the output: the library holds no mg_xline_chunk.c, and xline_chunk > 0 must be refused
by name."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
SCALE = 0.8


def main():
    so, out = sys.argv[1], sys.argv[2]
    import multigrid_petsc_amd._lib as loader
    lib = ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)
    loader._cache["mgk"] = lib
    loader._cache["mgpetsc"] = lib
    import rhs_cases
    from multigrid_petsc_amd.solver import MgError, Solver
    if out == "--unlinked":
        for pc in ("xline", "altline"):
            try:
                Solver(2, 33, 4, v=(3, 3), maxiter=20, scale=SCALE, pc_type=pc, xline_chunk=16)
                raise SystemExit("xline_chunk=16 was accepted by a build without mg_xline_chunk.c")
            except MgError as e:
                assert "mg_xline_chunk.c is not linked" in str(e), str(e)
            s = Solver(2, 33, 4, v=(3, 3), maxiter=20, scale=SCALE, pc_type=pc, xline_chunk=0)      # off: served as before
            s.set_rhs_problem()
            s.solve()
            s.close()
        return
    for f in (lib.mock_chunk_calls, lib.mock_xchunk_calls):
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int]
    lib.mock_xline_log.restype = ctypes.c_char_p
    res = {}
    for key in sys.argv[3:]:
        pc, xc, yc, case = key.split(";")
        xc, yc = int(xc), int(yc)
        f = case.split(",")
        npts, levels, mesh, rhs = int(f[0]), int(f[1]), int(f[2]), f[3]

        def make(**kw):
            kw.setdefault("xline_chunk", xc)
            if kw["xline_chunk"] is None:
                del kw["xline_chunk"]
            s = Solver(2, npts, levels, v=(3, 3), maxiter=100, scale=SCALE, mesh=mesh, pc_type=pc, line_chunk=yc, **kw)
            if rhs == "manufactured":
                s.set_rhs_problem()
            else:
                s.set_rhs(rhs_cases.uniform(2, npts, int(rhs.split(":")[1])))
            return s

        k = key + ":"
        s = make()
        lib.mock_xline_log_clear()
        lib.mock_chunk_calls_reset()
        lib.mock_xchunk_calls_reset()
        it = s.solve()
        res[k + "it"], res[k + "rn"], res[k + "u"], res[k + "bnorm"] = it, s.rnorm, s.solution(), s.bnorm
        log = lib.mock_xline_log().decode()
        res[k + "calls"] = np.array([log.count(ch) for ch in "fbFB"] + [lib.mock_chunk_calls(q) for q in range(4)] + [lib.mock_xchunk_calls(q) for q in range(4)])
        s.reset()
        assert s.solve() == it and np.array_equal(s.rnorm, res[k + "rn"]) and np.array_equal(s.solution(), res[k + "u"]), "reset + solve differs"
        s.close()
        for tag, kw in (("graph0", dict(graph=0)), ("fuse0", dict(fuse=0))) + ((("nokw", dict(xline_chunk=None)),) if xc == 0 else ()):
            s = make(**kw)
            res[k + tag + "_it"], res[k + tag + "_rn"], res[k + tag + "_u"] = s.solve(), s.rnorm, s.solution()
            s.close()
    # what xline_chunk is not built for is refused at creation, with the reason; the refusals of the line smoothers and of line_chunk stay
    for kw, msg in ((dict(pc_type="xline", xline_chunk=-16), "xline_chunk must be"), (dict(pc_type="xline", xline_chunk=8), "xline_chunk must be"),
                    (dict(pc_type="altline", xline_chunk=24), "xline_chunk must be"), (dict(pc_type="altline", xline_chunk=1), "xline_chunk must be"),
                    (dict(pc_type="jacobi", xline_chunk=16), "not jacobi or yline"), (dict(pc_type="yline", xline_chunk=16), "not jacobi or yline"),
                    (dict(pc_type="xline", xline_chunk=16, line_chunk=8), "not jacobi or xline"),
                    (dict(pc_type="xline", xline_chunk=16, precision="mixed"), "not mixed precision"),
                    (dict(pc_type="altline", xline_chunk=16, ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev")):
        try:
            Solver(2, 33, 4, v=(3, 3), maxiter=20, scale=SCALE, **kw)
            raise SystemExit(f"{kw} was accepted")
        except MgError as e:
            assert msg in str(e), str(e)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
