"""Solver(pc_type="xline" / "altline", xline_chunk=c, scale=0.8) on the GPU against tests/xchunkline_reference.py (the numpy statement of the
cycle with its x-line sweeps solved in chunks, over the oracle's assembled rows and transfers): the solves of tests/test_xchunkline_cpu.py on
the real libraries.

  cases          xline and altline at npts 65 and 129 on meshes 0, 1 and 2 with c = 16 and c = 32 (at npts 65 the levels 63 and 31 run the four
                 passes -- inside the recorded coarse-level graph too -- and 15, 7, 3, 1 the plain two), and altline with line_chunk set as
                 well (tests/chunkline_reference.py for the chunked y sweeps); the right-hand sides are those of the CPU tier
  checks         line_reference.compare: the same cycle count (the reference's stop decision is clear of rounding: last norm <= 0.8, the one
                 before >= 1.5 rtol ||b||; the four x-line cases on mesh 1 as in the CPU tier), the history within 1e-12 of rnorm[0], u bit for
                 bit; reset() + solve() and graph=0 repeat the bits
  xline_chunk=0  the plain reference, and the bits of a solver built without the keyword
  refusals       xline_chunk < 0 or no multiple of 16; xline_chunk > 0 with pc_type jacobi or yline"""
import numpy as np
import pytest

import line_reference as LR
import xchunkline_reference as XC
from oracle import Oracle
from test_xchunkline_cpu import BOTH, SOLVES, ZERO, _compare, _key

pytestmark = pytest.mark.gpu
GPU_SOLVES = [k for k in SOLVES + BOTH if k[3][0] in (65, 129)]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _solver(pc, case, **kw):
    import rhs_cases
    from multigrid_petsc_amd.solver import Solver
    npts, levels, mesh, rhs = case
    s = Solver(2, npts, levels, v=(3, 3), maxiter=100, scale=LR.SCALE, mesh=mesh, pc_type=pc, **kw)
    if rhs == "manufactured":
        s.set_rhs_problem()
    else:
        s.set_rhs(rhs_cases.uniform(2, npts, int(rhs.split(":")[1])))
    return s


def _check(ref, pc, case, tag, **kw):
    s = _solver(pc, case, **kw)
    it = s.solve()
    rn, u, bn = s.rnorm, s.solution(), s.bnorm
    m = min(len(rn), len(ref["rnorm"]))
    print(f"{tag} {LR.case_key(case)}: {it} cycles (reference {ref['iters']}), max history diff / rnorm[0] = "
          f"{np.abs(rn[:m] - ref['rnorm'][:m]).max() / ref['rnorm'][0]:.2e}, u differs in {int(np.sum(u != ref['u']))} of {u.size}")
    _compare(pc, case, ref, it, rn, u, bn)
    # again on the same solver: the recorded coarse-level graph is replayed from fresh state
    s.reset()
    assert s.solve() == it and np.array_equal(s.rnorm, rn) and np.array_equal(s.solution(), u)
    s.close()
    t = _solver(pc, case, graph=0, **kw)
    assert t.solve() == it and np.array_equal(t.rnorm, rn) and np.array_equal(t.solution(), u), "graph=0"
    t.close()
    return it, rn, u


@pytest.mark.parametrize("pc,xc,yc,case", GPU_SOLVES, ids=[_key(*k) for k in GPU_SOLVES])
def test_chunked_xline_solve_equals_the_reference(orc, pc, xc, yc, case):
    _check(XC.reference(orc, case, pc, xc, yc), pc, case, f"{pc} xc={xc} yc={yc}", xline_chunk=xc, line_chunk=yc)


@pytest.mark.parametrize("pc,xc,yc,case", ZERO, ids=[_key(*k) for k in ZERO])
def test_xline_chunk_0_is_the_plain_solve(orc, pc, xc, yc, case):
    it, rn, u = _check(XC.reference(orc, case, pc, 0, yc), pc, case, "xc=0", xline_chunk=0, line_chunk=yc)
    s = _solver(pc, case, line_chunk=yc)                     # without the keyword
    assert s.solve() == it and np.array_equal(s.rnorm, rn) and np.array_equal(s.solution(), u)
    s.close()


def test_what_xline_chunk_is_not_built_for_is_refused():
    from multigrid_petsc_amd.solver import MgError, Solver
    for kw, msg in ((dict(pc_type="xline", xline_chunk=-16), "xline_chunk must be"), (dict(pc_type="altline", xline_chunk=8), "xline_chunk must be"),
                    (dict(pc_type="altline", xline_chunk=40), "xline_chunk must be"),
                    (dict(pc_type="jacobi", xline_chunk=16), "not jacobi or yline"), (dict(pc_type="yline", xline_chunk=16), "not jacobi or yline")):
        with pytest.raises(MgError, match=msg):
            Solver(2, 33, 4, v=(3, 3), maxiter=20, scale=LR.SCALE, **kw)
