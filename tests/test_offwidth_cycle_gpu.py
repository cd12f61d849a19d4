"""Whole solves on the GPU at npts - 1 = 3 * 2^k.  mg_solver_create takes every npts with npts - 1 divisible by 2^(levels-1) and odd level widths; every
other cycle test takes npts = 2^k + 1.  Here the level widths are 5, 11, 23, 47, 95, 191, 383, 767, 1535: short rows, partial wave rows, and rows of
three / six whole waves that run in a block of four / eight.  Each case is compared against the reference its own cycle test uses:

  3-D point Jacobi    npts 25, 49, 97, 193; fp64 and mixed precision; the default fusions, fuse=0 and pair_min_n=7; solved to the tolerance against
                      Oracle.vcycle / vcycle_mixed (tests/offwidth_cases.py: count, history to 1e-12, u bit for bit) -- tests/test_vcycle_gpu.py
  z-slab ranks        2 and 3 loopback ranks at npts 97 (tests/test_multirank_gpu.py), against the oracle
  3-D, 383 wide       Solver(3, 385, 2, v=(2, 2)), one cycle with the default pair_min_n: the two-sweep pass of level 0 on rows of three waves
  2-D point Jacobi    npts 97, 193, 385, 1537; meshes 0, 1, 2; Richardson and Chebyshev: five cycles each with its norm, and on the uniform mesh
                      the solve to the tolerance -- tests/test_vcycle_gpu.py, tests/test_cheby_cycle_gpu.py
  2-D line smoothers  yline, xline, altline with and without line_chunk, xline_chunk and line_tail, and rbgs: four cycles each with its norm against
                      the numpy cycles of tests/xline_reference.py, chunkline_reference.py, xchunkline_reference.py and rbgs_reference.py (history
                      within 1e-12 of rnorm[0], u bit for bit: the bars of their compare())
  FMG, GMRES          tests/fmg_reference.py and tests/gmres_reference.py, with the assertions of tests/test_fmg_gpu.py and test_gmres_solve_gpu.py

The cases with a fixed count run solve() with maxiter = count and a tolerance that is never met, so every cycle's norm is monitored and compared; their
references (numpy, row by row) stay at a few cycles."""
import time

import numpy as np
import pytest

import chunkline_reference as CR
import gmres_reference as G
import line_reference as LR
import offwidth_cases as OW
import rbgs_reference as RB
import xchunkline_reference as XC
import xline_reference as XR
from fmg_reference import FmgRef
from oracle import Oracle
from test_multirank_gpu import _solve_ranks

pytestmark = pytest.mark.gpu
LINE_CYCLES = 4


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _Solver():
    from multigrid_petsc_amd.solver import Solver
    return Solver


@pytest.mark.parametrize("kw", OW.VARIANTS_3D, ids=["default", "fuse0", "pair7"])
@pytest.mark.parametrize("precision", ["fp64", "mixed"])
@pytest.mark.parametrize("npts", [25, 49, 97, 193])
def test_3d_solve_equals_the_oracle(orc, npts, precision, kw):
    OW.check3d(_Solver(), orc, npts, precision, kw)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("P", [2, 3])
def test_loopback_slab_ranks_at_97(orc, P):
    OW.check_slabs(_solve_ranks, orc, P, 97)


def test_one_cycle_at_385_cubed_with_the_default_pair_threshold(orc):
    """level 0 is 383 wide, three whole waves per row, and n >= pair_min_n = 255: with v = (2, 2) both smoothings of level 0 are one two-sweep pass
    (mgk_jacobi2_f64 and the norm forms where mgk_jacobi2_sumsq_ok_f64 offers them).  One cycle from the manufactured right-hand side"""
    t0 = time.time()
    s = _Solver()(3, 385, 2, v=(2, 2), maxiter=1, rtol=OW.NEVER, scale=OW.SC3)
    try:
        s.set_rhs_problem()
        it = s.solve()
        rn, u = s.rnorm, s.solution()
    finally:
        s.close()
    t1 = time.time()
    ref = orc.vcycle(3, 385, 2, 2, 2, maxiter=1, rtol=OW.NEVER, scale=OW.SC3)
    print(f"\n385^3, one cycle: product {t1 - t0:.1f} s, oracle {time.time() - t1:.1f} s")
    OW.same(ref, it, rn, u, "3-D npts=385 levels=2 v=(2,2)")


@pytest.mark.parametrize("cheby", [False, True], ids=["richardson", "chebyshev"])
@pytest.mark.parametrize("mesh", [0, 1, 2])
@pytest.mark.parametrize("npts", [97, 193, 385, 1537])
def test_2d_five_cycles_equal_the_oracle(orc, npts, mesh, cheby):
    OW.check2d(_Solver(), orc, npts, mesh, cheby, 5, {})


@pytest.mark.parametrize("kw", [{}, {"fuse": 0}, {"pair_min_n": 7}], ids=["default", "fuse0", "pair7"])
@pytest.mark.parametrize("npts", [97, 193, 385, 1537])
def test_2d_solve_on_the_uniform_mesh_equals_the_oracle(orc, npts, kw):
    OW.check2d(_Solver(), orc, npts, 0, False, 0, kw)


# (pc_type, npts, mesh, solver keywords): the reference is the hierarchy class that states the same sweeps
LINE_CASES = [(pc, npts, mesh, {}) for pc in ("yline", "xline", "altline") for npts in (97, 193) for mesh in (0, 1, 2)] + [
    ("altline", 385, 1, {}), ("yline", 385, 2, {}), ("xline", 385, 0, {}),
    ("yline", 193, 1, {"line_chunk": 16}), ("altline", 385, 1, {"line_chunk": 16}), ("xline", 193, 1, {"xline_chunk": 16}),
    ("altline", 385, 2, {"xline_chunk": 32, "line_chunk": 16}), ("altline", 1537, 1, {"xline_chunk": 128, "line_chunk": 128}),
    ("yline", 193, 1, {"line_tail": 1}), ("xline", 97, 2, {"line_tail": 1}), ("altline", 385, 1, {"line_tail": 1}),
    ("altline", 193, 0, {"line_tail": 1, "line_chunk": 16, "xline_chunk": 16}),
    ("rbgs", 97, 0, {}), ("rbgs", 193, 1, {}), ("rbgs", 385, 2, {}), ("rbgs", 769, 0, {})]
_LINE_REF = {}


def _line_reference(orc, pc, npts, mesh, kw):
    yc, xc = kw.get("line_chunk", 0), kw.get("xline_chunk", 0)
    key = (pc, npts, mesh, yc, xc)                         # (line_tail changes no bit: the same reference)
    if key not in _LINE_REF:
        L = OW.levels_of(npts)
        if pc == "rbgs":
            h = RB.Hierarchy(orc, npts, L, mesh)
            _LINE_REF[key] = RB.solve(h, h.rhs(), 1.0, v=(2, 2), rtol=0.0, maxiter=LINE_CYCLES)
        else:
            if xc:
                h = XC.Hierarchy(orc, npts, L, mesh, pc, xc, yc)
            elif yc:
                h = (CR.AltHierarchy if pc == "altline" else CR.Hierarchy)(orc, npts, L, mesh, yc)
            else:
                h = XR.Hierarchy(orc, npts, L, mesh, pc)
            _LINE_REF[key] = LR.solve(h, h.rhs(), LR.SCALE, v=(3, 3), rtol=0.0, maxiter=LINE_CYCLES)
    return _LINE_REF[key]


@pytest.mark.parametrize("pc,npts,mesh,kw", LINE_CASES, ids=[f"{pc}-{n}-mesh{m}" + "".join(f"-{k}{v}" for k, v in kw.items()) for pc, n, m, kw in LINE_CASES])
def test_2d_line_and_red_black_cycles_equal_their_references(orc, pc, npts, mesh, kw):
    ref = _line_reference(orc, pc, npts, mesh, kw)
    assert ref["iters"] == LINE_CYCLES
    rb = pc == "rbgs"
    s = _Solver()(2, npts, OW.levels_of(npts), v=(2, 2) if rb else (3, 3), maxiter=LINE_CYCLES, rtol=OW.NEVER, scale=1.0 if rb else LR.SCALE, mesh=mesh,
                  pc_type=pc, **kw)
    try:
        s.set_rhs_problem()
        it = s.solve()
        rn, u, bn = s.rnorm, s.solution(), s.bnorm
        if kw.get("line_tail"):
            assert s.tail_level > 0, "the LDS tail did not run"
    finally:
        s.close()
    assert it == LINE_CYCLES and len(rn) == it + 1 and abs(bn - ref["bnorm"]) <= 1e-13 * ref["bnorm"]
    assert np.abs(rn - ref["rnorm"]).max() <= 1e-12 * ref["rnorm"][0], np.abs(rn - ref["rnorm"]).max() / ref["rnorm"][0]
    assert np.array_equal(u, ref["u"]), f"u differs in {int(np.sum(u != ref['u']))} of {u.size}"


@pytest.mark.parametrize("dim,npts,v,nu", [(2, 97, (3, 3), 1), (2, 385, (3, 3), 2), (2, 1537, (1, 2), 1), (3, 49, (3, 3), 1), (3, 97, (3, 3), 2), (3, 193, (1, 2), 1)])
def test_fmg_equals_the_restatement(orc, dim, npts, v, nu):
    sc = OW.SC3 if dim == 3 else OW.SC2
    s = _Solver()(dim, npts, OW.levels_of(npts), v=v, scale=sc, maxiter=50)
    try:
        s.set_rhs_problem()
        assert s.fmg(nu) == 1
        u, rn = s.solution(), s.rnorm
    finally:
        s.close()
    f = FmgRef(orc, dim, npts, OW.levels_of(npts), v, sc)
    ref = f.fmg(nu)
    assert np.array_equal(u, ref), f"FMG({nu}) u0, dim={dim} npts={npts} v={v}"
    assert len(rn) == 2
    assert abs(rn[0] / f.rnorm_of(f.zeros(0)) - 1.0) <= 1e-12 and abs(rn[1] / f.rnorm_of(ref) - 1.0) <= 1e-12


@pytest.mark.parametrize("dim,npts,mesh,restart,scale", [(2, 97, 0, 30, 0.8), (2, 385, 2, 5, 0.8), (3, 49, 0, 30, 1.0), (3, 97, 0, 30, 0.8)])
def test_solve_gmres_equals_the_reference(orc, dim, npts, mesh, restart, scale):
    """the bars of tests/test_gmres_solve_gpu.py: the count of both dot variants of the reference (their stop decision clear of rounding), x and the
    history within 100 times the distance between the two variants.  (The cases are those of the sizes tried whose reference stops clear of the
    threshold: on mesh 1 at 97, 193 and 385 the last estimate lands within 20 % of it.)"""
    levels, rtol = OW.levels_of(npts), 1.0e-7
    op = G.Operators(orc, dim, npts, levels, mesh, scale)
    b = op.rhs()
    refs = [G.gmres(op, b, restart, rtol=rtol, maxiter=100, dot=d) for d in ("np", "ld")]
    op.close()
    for r in refs:
        last, before = G.margins(r, rtol)
        assert last <= 0.8 and before >= 1.5, (last, before)
    assert refs[0]["iters"] == refs[1]["iters"]
    s = _Solver()(dim, npts, levels, v=(3, 3), maxiter=100, scale=scale, mesh=mesh, rtol=rtol)
    try:
        s.set_rhs_problem()
        it = s.solve_gmres(restart)
        x, rn = s.solution(), s.rnorm
        assert it == refs[0]["iters"], (it, refs[0]["iters"])
        assert len(rn) == it + 1 and abs(s.bnorm - refs[0]["bnorm"]) <= 1e-13 * refs[0]["bnorm"] and rn[0] == s.bnorm
    finally:
        s.close()
    bound = max(100.0 * G.delta(refs[0], refs[1]), 1e-13)
    dist = min(G.distance(x, rn, r) for r in refs)
    assert dist <= bound, (dist, bound)
