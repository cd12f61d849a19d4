"""The FMG interpolation passes and the prolongation passes they are built on, for the PMC (HBM traffic) passes of rocprofv3:
mgk_interp_jacobi2_f64 / mgk_prolong_jacobi2_f64 at n^3 (default 1023) and mgk_interp_jacobi3_2d_f64 / mgk_prolong_jacobi3_2d_f64 at m^2
(default 4095), three launches each.  Run under
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- python3 tools/pmc_fmg.py
and again with --pmc WRITE_SIZE (the two do not fit one pass on gfx950); tools/pmc_summary.py DIR averages the counters per kernel."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_petsc_amd.mgk import Mgk  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1023
m2 = int(sys.argv[2]) if len(sys.argv) > 2 else 4095
SC = 6.0 / 7.0
m = Mgk(0)
L = m.L
rng = np.random.default_rng(0)


def filled(g, seed):
    """a field with smooth non-zero values (separable product of random rows)"""
    r = [m.upload(rng.uniform(-1, 1, max(g.nx, g.ny, g.nz))) for _ in range(3)]
    f = m.field(g)
    m._chk(L.mgk_fill_separable_f64(m.ctx, C.byref(g), r[0], r[1], r[2] if g.dim == 3 else None, f, None))
    m.sync()
    for p in r:
        m.free(p)
    return f


g, gc = m.geom(3, n), m.geom(3, (n - 1) // 2)
b, u, uc, out = filled(g, 1), filled(g, 2), filled(gc, 3), m.field(g)
h = 1.0 / (n + 1)
c = 1.0 / (h * h)
As = [c] * 7
As[3] = -6 * c
coef, dinv = m.coef(As), 1.0 / As[3]
for _ in range(3):
    m._chk(L.mgk_interp_jacobi2_f64(m.ctx, C.byref(g), C.byref(gc), coef, dinv, SC, b, uc, out, None))
    m._chk(L.mgk_prolong_jacobi2_f64(m.ctx, C.byref(g), C.byref(gc), coef, dinv, SC, b, uc, u, out, None))
m.sync()
for p in (b, u, uc, out):
    m.free(p)

g2, gc2 = m.geom(2, m2), m.geom(2, (m2 - 1) // 2)
b, u, uc, out = filled(g2, 4), filled(g2, 5), filled(gc2, 6), m.field(g2)
h = 1.0 / (m2 + 1)
c = 1.0 / (h * h)
As2 = [c, c, -4 * c, c, c]
coef2, dinv2 = m.coef(As2), 1.0 / As2[2]
for _ in range(3):
    m._chk(L.mgk_interp_jacobi3_2d_f64(m.ctx, C.byref(g2), C.byref(gc2), coef2, dinv2, 0.8, b, uc, out, None))
    m._chk(L.mgk_prolong_jacobi3_2d_f64(m.ctx, C.byref(g2), C.byref(gc2), coef2, dinv2, 0.8, None, None, b, uc, u, out, None))
m.sync()
for p in (b, u, uc, out):
    m.free(p)
m.close()
print("pmc_fmg done")
