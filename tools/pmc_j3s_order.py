"""The two stacked level-0 passes (k_jacobi3s<4,1> and <4,0,PRO>) for the counter runs of rocprofv3 (profiles/stacked_l2/README.md): one launch
of each per setting, in the order printed, so that the rows of the counter csv are told apart by their dispatch order.
Run under:  rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- python3 tools/pmc_j3s_order.py [--variants V,V,...]
and again with the other counters (a run of its own each, without tracing).
Settings: the full 1023^3 box under the default tuning and under every variant given; then the SINGLE-ROUND box 1023 x 727 x 1023 with one
z chunk (9 x 28 = 252 tiles: one round of the 256 CUs, every block starts together) under the same tunings."""
import ctypes as C
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_petsc_amd.mgk import Mgk

variants = [-1]
if "--variants" in sys.argv:
    variants += [int(v) for v in sys.argv[sys.argv.index("--variants") + 1].split(",") if v]
m = Mgk(0); L = m.L
rng = np.random.default_rng(0)
r1 = [m.upload(rng.uniform(-1, 1, 1023)) for _ in range(3)]
rc = [m.upload(rng.uniform(-1, 1, 511)) for _ in range(3)]
c = float(1024 ** 2)
As = [c] * 7; As[3] = -6 * c
coef = m.coef(As); dinv = 1.0 / As[3]
ss = C.c_double()
k = 0
for (nx, ny, nz), zc in (((1023, 1023, 1023), -1), ((1023, 727, 1023), 1023)):
    g, gc = m.geom(3, nx, ny, nz), m.geom(3, (nx - 1) // 2, (ny - 1) // 2, (nz - 1) // 2)
    G, GC = C.byref(g), C.byref(gc)
    u, b, out, uc = m.field(g), m.field(g), m.field(g), m.field(gc)
    m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[0], r1[1], r1[2], u, None))
    m._chk(L.mgk_fill_separable_f64(m.ctx, G, r1[2], r1[0], r1[1], b, None))
    m._chk(L.mgk_fill_separable_f64(m.ctx, GC, rc[0], rc[1], rc[2], uc, None))
    m.sync()
    for v in variants:
        L.mgk_set_tuning(v, zc)
        try:
            m._chk(L.mgk_jacobi3_sumsq_f64(m.ctx, G, coef, dinv, 6.0 / 7.0, b, u, out, C.byref(ss), None))
            m._chk(L.mgk_prolong_jacobi3_f64(m.ctx, G, GC, coef, dinv, 6.0 / 7.0, b, uc, u, out, None))
        finally:
            L.mgk_set_tuning(-1, -1)
        m.sync()
        print(f"launches {k} (k_jacobi3s<4,1>) and {k + 1} (k_jacobi3s<4,0,PRO>) of k_jacobi3s: {nx} x {ny} x {nz}, variant {v}, zchunk {zc}, "
              f"{nx * ny * nz} unknowns", flush=True)
        k += 2
    for p in (u, b, out, uc):
        m.free(p)
m.close()
