"""Solver(..., line_tail=1) on the GPU: the coarse levels of a line cycle inside ONE kernel (mgk_tail_cycle_line_f64) against the numpy
references of the line cycles (tests/xline_reference.py, tests/line_reference.py) and against the same solve made launch by launch.

  cases          every case of XR.CASES with npts <= 129 and the y cases of LR.CASES (all with a stop decision clear of rounding)
  checks         the pinned count, the history within 1e-12 of rnorm[0], u bit for bit (XR.compare / LR.compare); count, history and u
                 EQUAL (np.array_equal) to the same solve with line_tail=0; tail_level 1, and 0 with line_tail=0; graph=0 gives the same
                 bits; reset() + solve() repeats them
  other counts   v = (2, 1) and (1, 2) on (altline, 33, 5, 2)
  level rule     npts 257, 8 levels: the tail starts below every chunk period that applies to the pc_type, and each configuration is
                 bit-identical to itself with line_tail=0
  refusals       line_tail=2; line_tail=1 with point Jacobi; levels=2 at npts 257 leaves tail_level 0 and still solves"""
import numpy as np
import pytest

import line_reference as LR
import xline_reference as XR
from oracle import Oracle

pytestmark = pytest.mark.gpu
CASES = [c for c in XR.CASES if c[1] <= 129] + [("yline",) + c + (None,) for c in LR.CASES]
IDS = [XR.xcase_key(c) for c in CASES]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _solver(case, v=(3, 3), maxiter=100, **kw):
    import rhs_cases
    from multigrid_petsc_amd.solver import Solver
    pc, npts, levels, mesh, rhs = case[:5]
    s = Solver(2, npts, levels, v=v, maxiter=maxiter, scale=XR.SCALE, mesh=mesh, pc_type=pc, **kw)
    if rhs == "manufactured":
        s.set_rhs_problem()
    else:
        s.set_rhs(rhs_cases.uniform(2, npts, int(rhs.split(":")[1])))
    return s


def _solve(case, **kw):
    s = _solver(case, **kw)
    out = (s.solve(), s.rnorm, s.solution(), s.bnorm, s.tail_level)
    s.close()
    return out


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_solve_with_the_tail_equals_the_reference_and_the_launches(orc, case):
    ref = LR.reference(orc, case[1:5]) if case[0] == "yline" else XR.reference(orc, case)
    if case[5] is not None:
        assert ref["iters"] == case[5]
    s = _solver(case, line_tail=1)
    it = s.solve()
    rn, u, bn = s.rnorm, s.solution(), s.bnorm
    m = min(len(rn), len(ref["rnorm"]))
    print(f"{XR.xcase_key(case)}: {it} cycles (reference {ref['iters']}), max history diff / rnorm[0] = "
          f"{np.abs(rn[:m] - ref['rnorm'][:m]).max() / ref['rnorm'][0]:.2e}, u differs in {int(np.sum(u != ref['u']))} of {u.size}")
    XR.compare(ref, it, rn, u, bn)
    assert s.tail_level == 1
    # again on the same solver: the recorded coarse-level graph, the tail launch in it, is replayed from fresh state
    s.reset()
    assert s.solve() == it and np.array_equal(s.rnorm, rn) and np.array_equal(s.solution(), u)
    s.close()
    off = _solve(case, line_tail=0)
    assert off[4] == 0 and _same(off, (it, rn, u)), "line_tail=0"
    g0 = _solve(case, line_tail=1, graph=0)
    assert g0[4] == 1 and _same(g0, (it, rn, u)), "graph=0"


@pytest.mark.parametrize("v", [(2, 1), (1, 2)])
def test_other_sweep_counts(orc, v):
    case = ("altline", 33, 5, 2, "manufactured")
    h = XR.Hierarchy(orc, 33, 5, 2, "altline")
    ref = XR.solve(h, h.rhs(), XR.SCALE, v=v, rtol=XR.RTOL, maxiter=100)
    on, off = _solve(case, v=v, line_tail=1), _solve(case, v=v, line_tail=0)
    print(f"v = {v}: {on[0]} cycles (reference {ref['iters']})")
    assert on[4] == 1 and off[4] == 0 and _same(on, off)
    assert on[0] == ref["iters"] and np.array_equal(on[2], ref["u"])
    assert np.abs(on[1] - ref["rnorm"]).max() <= 1e-12 * ref["rnorm"][0]


# npts 257, 8 levels: n = 255, 127, 63, 31, 15, 7, 3, 1 on the levels 0 .. 7
@pytest.mark.parametrize("pc,kw,level", [("altline", dict(line_chunk=32), 3), ("altline", dict(xline_chunk=16), 4),
                                         ("altline", dict(line_chunk=32, xline_chunk=16), 4), ("yline", dict(line_chunk=64), 2)],
                         ids=["y32", "x16", "y32x16", "yline-y64"])
def test_the_tail_starts_below_every_chunk_period_that_applies(pc, kw, level):
    case = (pc, 257, 8, 1, "manufactured")
    on, off = _solve(case, line_tail=1, **kw), _solve(case, line_tail=0, **kw)
    assert on[4] == level and off[4] == 0
    assert _same(on, off), kw
    assert on[0] >= 1 and on[1][-1] <= XR.RTOL * on[3]


def test_refusals_and_fall_backs():
    from multigrid_petsc_amd.solver import MgError, Solver
    with pytest.raises(MgError, match="line_tail must be 0 .off. or 1"):
        Solver(2, 33, 5, scale=XR.SCALE, pc_type="altline", line_tail=2)
    with pytest.raises(MgError, match="line_tail goes with the line smoothers"):
        Solver(2, 33, 5, scale=XR.SCALE, pc_type="jacobi", line_tail=1)
    # two levels at npts 257: nothing fits in LDS (n = 255, 127): accepted, the tail stays off, and it still solves
    case = ("altline", 257, 2, 0, "manufactured")
    on, off = _solve(case, maxiter=4, line_tail=1), _solve(case, maxiter=4, line_tail=0)
    assert on[4] == 0 and off[4] == 0 and on[0] == 4 and _same(on, off)
    assert on[1][-1] < on[1][0]
    # ... and with fuse=0 the tail is still used: line_tail is independent of the fuse bits
    s = _solver(("altline", 33, 5, 1, "manufactured"), line_tail=1, fuse=0)
    assert s.tail_level == 1
    s.close()
