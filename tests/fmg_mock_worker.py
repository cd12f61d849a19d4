"""Worker of tests/test_random_sessions_cpu.py: the four full-multigrid stand-ins of tests/mock_mgk_fmg.cpp called one by one through ctypes --
"device" memory of the stand-ins is host memory, so padded numpy arrays are the fields.  A process of its own: nothing of the test process
loads the mock library.  argv: library, output .npz.  Saves every input and output (compact lexicographic fields) for the test to compare
with tests/fmg_reference.py:
  tail:<dim>:<nu>:<v0>:<v1>:{b,u}    mgk_tail_fmg_f64 on the stacks 63 .. 1 (2-D) and 15 .. 1 (3-D), random right-hand side
  interp:<dim>:{b,uc,u}              mgk_interp_jacobi3_2d_f64 (2-D, 31 <- 15) / mgk_interp_jacobi2_f64 (3-D, 15 <- 7), random b and uc
and ghosts:<key> = 1 where the stand-in left every ghost cell of its output zero."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
TAIL = [(dim, nu, v) for dim in (2, 3) for nu in (1, 2) for v in ((3, 3), (1, 2), (5, 1))]
SCALE = {2: 0.8, 3: 6.0 / 7.0}
dp = C.POINTER(C.c_double)


def main():
    from multigrid_petsc_amd.mgk import Geom
    from oracle import Oracle
    L = C.CDLL(sys.argv[1])
    orc = Oracle()
    ctx = C.c_void_p()
    assert L.mgk_ctx_create(C.byref(ctx), 0) == 0

    def geom(dim, n):
        g = Geom()
        assert L.mgk_geom_init(C.byref(g), dim, n, n, n) == 0
        return g

    def interior(g):
        k, i, j = np.meshgrid(np.arange(g.nz), np.arange(g.ny), np.arange(g.nx), indexing="ij")
        return (g.org + (k * g.plane if g.dim == 3 else 0) + i * g.pitch + j).ravel()

    def field(g, compact=None):
        f = np.zeros(g.total)
        if compact is not None:
            f[interior(g)] = compact
        return f

    def ptr(a):
        return a.ctypes.data_as(dp)

    def stencils(dim, n0, nlev):
        As = [orc.level_stencil(dim, n0 + 2, l)[0] for l in range(nlev)]
        k7 = np.zeros(7 * nlev)
        for q in range(nlev):
            k7[7 * q:7 * q + len(As[q])] = As[q]
        return As, k7, np.array([1.0 / As[q][3 if dim == 3 else 2] for q in range(nlev)])

    res = {}

    def keep(key, g, out):
        res[key + ":u"] = out[interior(g)].copy()
        ghosts = out.copy()
        ghosts[interior(g)] = 0.0
        res["ghosts:" + key] = int(not ghosts.any())

    for dim, nu, (v0, v1) in TAIL:
        n0, nlev = (63, 6) if dim == 2 else (15, 4)
        rng = np.random.default_rng(9000 + 100 * dim + 10 * nu + v0)
        b = rng.uniform(-1, 1, n0 ** dim)
        g = geom(dim, n0)
        As, k7, di = stencils(dim, n0, nlev)
        n = (C.c_int * nlev)(*[(n0 + 1) // (1 << l) - 1 for l in range(nlev)])
        fb, fu = field(g, b), field(g)
        L.mgk_tail_fmg_f64.argtypes = [C.c_void_p, C.POINTER(Geom), C.c_int, C.POINTER(C.c_int), dp, dp, C.c_double, C.c_int, C.c_int, C.c_int, dp, dp, C.c_void_p]
        rc = L.mgk_tail_fmg_f64(ctx, C.byref(g), nlev, n, ptr(k7), ptr(di), SCALE[dim], v0, v1, nu, ptr(fb), ptr(fu), None)
        assert rc == 0, rc
        key = f"tail:{dim}:{nu}:{v0}:{v1}"
        res[key + ":b"] = b
        keep(key, g, fu)
    for dim, n in ((2, 31), (3, 15)):
        nc = (n - 1) // 2
        rng = np.random.default_rng(9500 + dim)
        b, uc = rng.uniform(-1, 1, n ** dim), rng.uniform(-1, 1, nc ** dim)
        g, gc = geom(dim, n), geom(dim, nc)
        As, k7, di = stencils(dim, n, 1)
        fb, fuc, fu = field(g, b), field(gc, uc), field(g)
        fu[:] = np.nan                                             # the old unew is never read
        fu[np.setdiff1d(np.arange(g.total), interior(g))] = 0.0
        f = L.mgk_interp_jacobi3_2d_f64 if dim == 2 else L.mgk_interp_jacobi2_f64
        f.argtypes = [C.c_void_p, C.POINTER(Geom), C.POINTER(Geom), dp, C.c_double, C.c_double, dp, dp, dp, C.c_void_p]
        if dim == 3:
            assert L.mgk_interp_jacobi2_ok_f64(C.byref(g), C.byref(gc)) == L.mgk_prolong_jacobi2_ok_f64(C.byref(g), C.byref(gc)) == 1
            g2, gc2 = geom(2, n), geom(2, nc)
            assert L.mgk_interp_jacobi2_ok_f64(C.byref(g2), C.byref(gc2)) == L.mgk_prolong_jacobi2_ok_f64(C.byref(g2), C.byref(gc2)) == 0
        rc = f(ctx, C.byref(g), C.byref(gc), ptr(k7), di[0], SCALE[dim], ptr(fb), ptr(fuc), ptr(fu), None)
        assert rc == 0, rc
        key = f"interp:{dim}"
        res[key + ":b"], res[key + ":uc"] = b, uc
        keep(key, g, fu)
    L.mgk_ctx_destroy(ctx)
    np.savez(sys.argv[2], **res)


if __name__ == "__main__":
    main()
