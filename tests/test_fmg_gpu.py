"""Full multigrid on the GPU (mg_solver_fmg / mg_solver_solve_fmg and its kernels) against the CPU oracle's step primitives.

Kernels: every new entry point equals the oracle's composition (a zeroed field + P uc, then the sweeps) bit for bit at the widths its
instances cover, writes nothing past the field (sentinels) and leaves the ghost cells zero:
  mgk_interp_jacobi2_f64     k_pj2r3<8|4, false, true>             3-D thin grids 1023 / 511 wide; other widths are refused (_ok_ = 0)
  mgk_interp_jacobi3_2d_f64  k_jacobi3_2d<true, true, false, ..>   2-D 4095 / 2047 (marching form), 1023 / 127 (short chunks)
  mgk_tail_fmg_f64           k_tail_fmg<double, 2|3>               2-D stacks 63 .. 1, 3-D 15 .. 1, nu = 1, 2
Solver: mg_solver_fmg's u0 equals tests/fmg_reference.py bit for bit (the kernels' path with v = (3, 3), the zeroed-field fallback
with v0 = 1); solve_fmg's iteration count and u equal the restatement's, its residual history agrees to 1e-12 (the device sums
of squares and the oracle's long double sums differ in order only); fmg + cycles(k) under the coarse-level graph; refusals; reset."""
import ctypes as C

import numpy as np
import pytest

from fmg_reference import FmgRef
from oracle import Oracle

pytestmark = pytest.mark.gpu
SC3, SC2 = 6.0 / 7.0, 0.8
SENT = 12345.678
NO_TAIL = 63 | 256 | 1024 | 2048 | 4096 | 8192 | 16384      # the default fuse bits without bit 9 (the tail kernel)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _host_mem_gib():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / 2 ** 20
    except OSError:
        pass
    return 0.0


class Out:
    """an output field of geometry g with zero ghosts and a sentinel tail past its allocation's end"""

    def __init__(self, mgk, g, tail=256):
        self.mgk, self.g, self.tail = mgk, g, tail
        init = np.zeros(g.total + tail)
        init[g.total:] = SENT
        self.p = mgk.upload(init)

    def check(self):
        raw = self.mgk.download(self.p, self.g.total + self.tail)
        inner = self.mgk.from_field(self.g, self.p)
        assert np.all(raw[self.g.total:] == SENT), "a write past the field"
        body = raw[:self.g.total]
        assert abs(np.abs(body).sum() - np.abs(inner).sum()) <= 1e-12 * max(np.abs(inner).sum(), 1e-300), "a ghost cell was written"
        return inner

    def free(self):
        self.mgk.free(self.p)


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nz", [(1023, 3), (1023, 9), (511, 5), (511, 9)])
def test_interp_jacobi2_3d_equals_the_oracle(mgk, orc, n, nz):
    rng = np.random.default_rng(7000 + n + nz)
    nc, nzc = (n - 1) // 2, (nz - 1) // 2
    As = orc.level_stencil(3, n + 2, 0)[0]
    b, uc = rng.uniform(-1, 1, n * n * nz), rng.uniform(-1, 1, nc * nc * nzc)
    g, gc = mgk.geom(3, n, n, nz), mgk.geom(3, nc, nc, nzc)
    db, duc = mgk.to_field(g, b), mgk.to_field(gc, uc)
    p = orc.prolong_add(3, n, uc, np.zeros(n * n * nz), nzf=nz, nzc=nzc)
    j1 = orc.jacobi(3, n, As, SC3, b, p, nz=nz)
    ref = orc.jacobi(3, n, As, SC3, b, j1, nz=nz)
    L = mgk.L
    assert L.mgk_interp_jacobi2_ok_f64(C.byref(g), C.byref(gc)) == 1
    for zc in (-1, 4):                                               # default chunking, and chunks of 4 planes
        L.mgk_set_tuning(-1, zc)
        o = Out(mgk, g)
        mgk._chk(L.mgk_interp_jacobi2_f64(mgk.ctx, C.byref(g), C.byref(gc), mgk.coef(As), 1.0 / As[3], SC3, db, duc, o.p, None))
        assert np.array_equal(o.check(), ref), f"mgk_interp_jacobi2_f64 n={n} nz={nz} zc={zc}"
        o.free()
    L.mgk_set_tuning(-1, -1)
    assert np.array_equal(mgk.from_field(g, db), b) and np.array_equal(mgk.from_field(gc, duc), uc)
    mgk.free(db); mgk.free(duc)


@pytest.mark.parametrize("n", [127, 255])
def test_interp_jacobi2_3d_refuses_other_widths(mgk, n):
    g, gc = mgk.geom(3, n, n, 5), mgk.geom(3, (n - 1) // 2, (n - 1) // 2, 2)
    assert mgk.L.mgk_interp_jacobi2_ok_f64(C.byref(g), C.byref(gc)) == 0
    o = Out(mgk, g)
    rc = mgk.L.mgk_interp_jacobi2_f64(mgk.ctx, C.byref(g), C.byref(gc), mgk.coef(np.ones(7)), 1.0, 1.0, o.p, o.p, o.p, None)
    assert rc != 0
    o.check()
    o.free()


@pytest.mark.parametrize("n", [4095, 2047, 1023, 127])
def test_interp_jacobi3_2d_equals_the_oracle(mgk, orc, n):
    rng = np.random.default_rng(7100 + n)
    nc = (n - 1) // 2
    As = orc.level_stencil(2, n + 2, 0)[0]
    b, uc = rng.uniform(-1, 1, n * n), rng.uniform(-1, 1, nc * nc)
    g, gc = mgk.geom(2, n), mgk.geom(2, nc)
    db, duc = mgk.to_field(g, b), mgk.to_field(gc, uc)
    u = orc.prolong_add(2, n, uc, np.zeros(n * n))
    for _ in range(3):
        u = orc.jacobi(2, n, As, SC2, b, u)
    o = Out(mgk, g)
    mgk._chk(mgk.L.mgk_interp_jacobi3_2d_f64(mgk.ctx, C.byref(g), C.byref(gc), mgk.coef(As), 1.0 / As[2], SC2, db, duc, o.p, None))
    assert np.array_equal(o.check(), u), f"mgk_interp_jacobi3_2d_f64 n={n}"
    assert np.array_equal(mgk.from_field(g, db), b) and np.array_equal(mgk.from_field(gc, duc), uc)
    o.free(); mgk.free(db); mgk.free(duc)


@pytest.mark.parametrize("dim,n0,nlev", [(2, 63, 6), (2, 31, 3), (3, 15, 4), (3, 7, 2)])
@pytest.mark.parametrize("nu", [1, 2])
def test_tail_fmg_equals_the_restatement(mgk, orc, dim, n0, nlev, nu):
    rng = np.random.default_rng(7200 + 10 * dim + n0 + nu)
    sc = SC3 if dim == 3 else SC2
    f = FmgRef(orc, dim, n0 + 1 + 1, nlev, (3, 3), sc, b0=rng.uniform(-1, 1, n0 ** dim))
    ref = f.fmg(nu)
    g = mgk.geom(dim, n0)
    db = mgk.to_field(g, f.b0)
    o = Out(mgk, g)
    n = (C.c_int * nlev)(*f.n)
    k7 = np.zeros(7 * nlev)
    for q in range(nlev):
        k7[7 * q:7 * q + len(f.As[q])] = f.As[q]
    di = np.array([1.0 / f.As[q][3 if dim == 3 else 2] for q in range(nlev)])
    mgk._chk(mgk.L.mgk_tail_fmg_f64(mgk.ctx, C.byref(g), nlev, n, k7.ctypes.data_as(C.POINTER(C.c_double)),
                                    di.ctypes.data_as(C.POINTER(C.c_double)), sc, 3, 3, nu, db, o.p, None))
    assert np.array_equal(o.check(), ref), f"mgk_tail_fmg_f64 dim={dim} n0={n0} nu={nu}"
    assert np.array_equal(mgk.from_field(g, db), f.b0)
    o.free(); mgk.free(db)


# ---------------------------------------------------------------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------------------------------------------------------------
def _solver(dim, npts, levels, v, **kw):
    from multigrid_petsc_amd.solver import Solver
    s = Solver(dim, npts, levels, v=v, scale=SC3 if dim == 3 else SC2, **kw)
    s.set_rhs_problem()
    return s


FMG_CASES = [(2, 129, 7, (3, 3), 1, -1), (2, 129, 7, (1, 2), 2, -1), (2, 129, 7, (3, 3), 2, NO_TAIL), (2, 65, 2, (3, 3), 1, -1),
             (2, 1025, 10, (3, 3), 1, -1), (2, 1025, 10, (3, 3), 2, -1), (2, 1025, 10, (1, 2), 1, -1),
             (2, 4097, 12, (3, 3), 1, -1), (2, 4097, 12, (1, 2), 2, -1),
             (3, 33, 5, (3, 3), 1, -1), (3, 33, 5, (1, 2), 2, -1), (3, 33, 5, (3, 3), 2, NO_TAIL), (3, 17, 2, (3, 3), 1, -1),
             (3, 129, 7, (3, 3), 1, -1), (3, 129, 7, (3, 3), 2, -1), (3, 129, 7, (1, 2), 1, -1),
             (3, 513, 9, (3, 3), 1, -1), (3, 513, 9, (3, 3), 2, -1), (3, 513, 9, (1, 2), 1, -1)]


@pytest.mark.parametrize("dim,npts,levels,v,nu,fuse", FMG_CASES)
def test_fmg_equals_the_restatement(orc, dim, npts, levels, v, nu, fuse):
    s = _solver(dim, npts, levels, v, fuse=fuse, maxiter=50)
    assert s.fmg(nu) == 1
    u, rn = s.solution(), s.rnorm
    s.close()
    f = FmgRef(orc, dim, npts, levels, v, SC3 if dim == 3 else SC2)
    ref = f.fmg(nu)
    assert np.array_equal(u, ref), f"FMG({nu}) u0, dim={dim} npts={npts} v={v}"
    assert len(rn) == 2
    assert abs(rn[0] / f.rnorm_of(f.zeros(0)) - 1.0) <= 1e-12 and abs(rn[1] / f.rnorm_of(ref) - 1.0) <= 1e-12


@pytest.mark.timeout(1500)
def test_fmg_headline_size(orc):
    """3-D 1025^3 (the headline grid): FMG(1) u0 against the restatement where the host has the memory for the oracle"""
    need, have = 90.0, _host_mem_gib()
    if have < need:
        pytest.skip(f"the oracle's FMG at 1023^3 needs ~{need:.0f} GiB of host memory, {have:.0f} GiB available")
    s = _solver(3, 1025, 10, (3, 3), maxiter=5)
    s.fmg(1)
    u = s.solution()
    s.close()
    assert np.array_equal(u, FmgRef(orc, 3, 1025, 10, (3, 3), SC3).fmg(1))


@pytest.mark.parametrize("dim,npts,levels,nu", [(2, 129, 7, 1), (2, 1025, 10, 2), (3, 33, 5, 1), (3, 129, 7, 2)])
def test_solve_fmg_equals_the_restatement(orc, dim, npts, levels, nu):
    """iteration count and u exactly; the residual history to 1e-12 (device sums of squares vs the oracle's long double sums: the
    reduction order differs)"""
    s = _solver(dim, npts, levels, (3, 3), maxiter=100)
    it = s.solve_fmg(nu)
    u, rn = s.solution(), s.rnorm
    assert s.solve_seconds > 0.0
    s.close()
    rit, ru, rrn = FmgRef(orc, dim, npts, levels, (3, 3), SC3 if dim == 3 else SC2).solve_fmg(nu, maxiter=100, rtol=1e-7)
    assert it == rit, (it, rit)
    assert np.abs(rn / rrn - 1.0).max() <= 1e-12
    assert np.array_equal(u, ru)


@pytest.mark.parametrize("dim,npts,levels", [(3, 129, 7), (2, 1025, 10), (2, 4097, 12)])
def test_fmg_then_cycles_under_the_coarse_graph(orc, dim, npts, levels):
    """a solve records the coarse-level graph; FMG then runs its stages below it (and may leave u / tmp of the level that feeds the graph
    swapped); the cycles that follow replay or re-record it: FMG + k cycles equal the restatement (graph on, lgraph > 0 at these sizes)"""
    k = 3
    s = _solver(dim, npts, levels, (3, 3), maxiter=100)
    s.solve()
    s.fmg(1)
    s.cycles(k)
    u, rn = s.solution(), s.rnorm
    s.close()
    ru, rrn = FmgRef(orc, dim, npts, levels, (3, 3), SC3 if dim == 3 else SC2).fmg_then_cycles(1, k)
    assert len(rn) == k + 2
    assert np.abs(rn / rrn - 1.0).max() <= 1e-12
    assert np.array_equal(u, ru)


def test_refused_configurations_leave_the_solver_usable(orc):
    from multigrid_petsc_amd.solver import MgError, Solver
    cases = [dict(dim=3, npts=33, levels=5, precision="mixed"),
             dict(dim=3, npts=33, levels=5, ksp_type="chebyshev", eigenvalues=(0.5, 2.0)),
             dict(dim=2, npts=65, levels=6, mesh=1),
             dict(dim=2, npts=65, levels=1)]
    for kw in cases:
        dim, npts, levels = kw.pop("dim"), kw.pop("npts"), kw.pop("levels")
        s = Solver(dim, npts, levels, v=(3, 3), maxiter=100, scale=SC3 if dim == 3 else SC2, **kw)
        s.set_rhs_problem()
        for fn in (s.fmg, s.solve_fmg):
            with pytest.raises(MgError, match=r"rc=-?\d+: mg_solver_fmg: (built for|needs)"):
                fn(1)
        it = s.solve()                                              # still usable: the refusal touched nothing
        assert it > 0 and np.isfinite(s.rnorm).all()
        s.close()
    # nu < 1
    s = _solver(2, 65, 6, (3, 3), maxiter=100)
    with pytest.raises(MgError, match="nu must be"):
        s.fmg(0)
    s.close()


def test_refused_on_two_loopback_ranks(orc):
    from multigrid_petsc_amd.comm import LoopbackWorld
    from multigrid_petsc_amd.solver import MgError, Solver
    ref = orc.vcycle(3, 65, 6, 3, 3, maxiter=100, scale=SC3)
    w = LoopbackWorld(2)

    def run(r, h):
        s = Solver(3, 65, 6, v=(3, 3), maxiter=100, scale=SC3, rank=r, nranks=2, comm=h)
        s.set_rhs_problem()
        try:
            s.fmg(1)
            return "accepted"
        except MgError as e:
            msg = str(e)
        it = s.solve()
        s.close()
        return msg, it

    try:
        res = w.run(run)
    finally:
        w.close()
    for msg, it in res:
        assert "nranks == 1" in msg
        assert it == ref["iters"]


@pytest.mark.parametrize("dim,npts,levels", [(2, 1025, 10), (3, 129, 7)])
def test_reset_after_fmg_solves_like_a_fresh_solver(dim, npts, levels):
    a = _solver(dim, npts, levels, (3, 3), maxiter=100)
    a.fmg(2)
    a.cycles(1)
    a.reset()
    ita = a.solve()
    ua, rna = a.solution(), a.rnorm
    a.close()
    b = _solver(dim, npts, levels, (3, 3), maxiter=100)
    itb = b.solve()
    ub, rnb = b.solution(), b.rnorm
    b.close()
    assert ita == itb and np.array_equal(rna, rnb) and np.array_equal(ua, ub)
