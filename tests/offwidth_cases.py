"""Whole solves at npts - 1 = 3 * 2^k (level widths 5, 11, 23, 47, 95, 191, 383, 767, 1535: rows that are no whole number of wave rows, or a number of
them that no block width matches): the cases and their comparison with the CPU oracle, shared by tests/test_offwidth_cycle_gpu.py (the product's
libraries, every size) and tests/test_offwidth_cycle_cpu.py (the same host logic over tests/mock_mgk.cpp, the small sizes).  Every case takes the
class Solver it is handed, so the two tiers run the same code.  The bars are those of tests/test_vcycle_gpu.py: iteration count equal, every norm of
the history within RTOL = 1e-12 of the oracle's, u bit for bit.  A reference is computed once per process and shared by the variants of a case.
Plain helper module (no fixtures).  Test infrastructure only."""
import numpy as np

RTOL = 1e-12
SC3, SC2 = 6.0 / 7.0, 0.8
EIG = (0.2, 2.0)
LEVELS = {13: 2, 25: 3, 49: 4, 97: 5, 193: 6, 385: 7, 769: 8, 1537: 9}          # the deepest hierarchy: down to 5 unknowns per axis
NEVER = 1e-30             # rtol of the fixed-count cases: maxiter cycles are run, every one with its monitored norm
VARIANTS_3D = ({}, {"fuse": 0}, {"pair_min_n": 7})
_REF = {}


def levels_of(npts):
    return LEVELS[npts]


def ref3d(orc, npts, precision):
    key = (3, npts, precision)
    if key not in _REF:
        L = LEVELS[npts]
        _REF[key] = (orc.vcycle(3, npts, L, 3, 3, maxiter=60, scale=SC3) if precision == "fp64" else
                     orc.vcycle_mixed(npts, L, 3, 3, maxiter=60, scale=SC3))
    return _REF[key]


def same(ref, it, rn, u, what):
    assert it == ref["iters"], f"{what}: {it} cycles, the oracle {ref['iters']}"
    rn = np.asarray(rn)
    assert rn.shape == ref["rnorm"].shape, what
    rel = np.abs(rn - ref["rnorm"]) / ref["rnorm"]
    assert rel.max() <= RTOL, f"{what}: residual history differs, max rel {rel.max():.3e}"
    assert np.array_equal(u, ref["u"]), f"{what}: u differs in {int(np.sum(u != ref['u']))} of {u.size} unknowns, max {np.abs(u - ref['u']).max():.3e}"


def check3d(Solver, orc, npts, precision, kw):
    """3-D, V(3,3), solved to the tolerance: the default fusions, the kernel-per-operation cycle (fuse=0), and pair_min_n=7 (the two-sweep and fused
    passes on every level down to 7^3, i.e. at the predicated widths)"""
    ref = ref3d(orc, npts, precision)
    assert 1 < ref["iters"] < 60
    s = Solver(3, npts, LEVELS[npts], v=(3, 3), maxiter=60, scale=SC3, precision=precision, **kw)
    try:
        s.set_rhs_problem()
        it = s.solve()
        same(ref, it, s.rnorm, s.solution(), f"3-D npts={npts} {precision} {kw}")
        assert abs(s.bnorm - ref["bnorm"]) <= RTOL * ref["bnorm"]
    finally:
        s.close()


def ref2d(orc, npts, mesh, cheby, cycles):
    key = (2, npts, mesh, cheby, cycles)
    if key not in _REF:
        kor = dict(ksp_type=1, emin=EIG[0], emax=EIG[1]) if cheby else dict(scale=SC2)
        kc = dict(maxiter=cycles, rtol=NEVER) if cycles else dict(maxiter=200)
        _REF[key] = orc.vcycle(2, npts, LEVELS[npts], 3, 3, use_csr=1 if mesh else 0, mesh=mesh, **kor, **kc)
    return _REF[key]


def check2d(Solver, orc, npts, mesh, cheby, cycles, kw):
    """2-D point Jacobi under Richardson or Chebyshev on mesh 0 / 1 / 2.  cycles > 0: that many cycles, every one with its norm (the stretched meshes
    take hundreds to converge under point Jacobi: the count of a solve to the tolerance is held on the uniform mesh, cycles == 0)"""
    ref = ref2d(orc, npts, mesh, cheby, cycles)
    assert ref["iters"] == cycles if cycles else 1 < ref["iters"] < 200
    kso = dict(ksp_type="chebyshev", eigenvalues=EIG) if cheby else dict(scale=SC2)
    kc = dict(maxiter=cycles, rtol=NEVER) if cycles else dict(maxiter=200)
    s = Solver(2, npts, LEVELS[npts], v=(3, 3), mesh=mesh, **kso, **kc, **kw)
    try:
        s.set_rhs_problem()
        it = s.solve()
        same(ref, it, s.rnorm, s.solution(), f"2-D npts={npts} mesh={mesh} {'chebyshev' if cheby else 'richardson'} cycles={cycles} {kw}")
    finally:
        s.close()


def check_slabs(solve_ranks, orc, P, npts, precision="fp64", dist_min_n=23):
    """P loopback z-slab ranks (tests/test_multirank_gpu.py::_solve_ranks): every rank the oracle's count and history (the norms are all-reduced
    block partials: 1e-12 as above), the concatenated slabs the oracle's u bit for bit"""
    ref = ref3d(orc, npts, precision)
    res = solve_ranks(P, npts, LEVELS[npts], SC3, 60, dist_min_n, precision=precision)
    planes = [r[4][0] for r in res]
    assert planes[0][0] == 0 and sum(p[1] for p in planes) == npts - 2, planes
    for r in res:
        assert r[0] == ref["iters"] and np.abs(r[1] / ref["rnorm"] - 1).max() <= RTOL
    u = np.concatenate([r[2] for r in res])
    assert np.array_equal(u, ref["u"]), f"P={P} npts={npts}: max diff {np.abs(u - ref['u']).max()}"
