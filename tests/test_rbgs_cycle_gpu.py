"""Solver(pc_type="rbgs") on the GPU against tests/rbgs_reference.py (numpy over the CPU oracle): whole solves, levels down to 1 x 1.

  cases      npts 17, 65, 129, 513 (the last: rows of several waves, several y chunks, the coarse-level graph) x meshes 0 / 1 / 2 x scale 1 and
             0.8 x v = (1,1), (2,2), (3,2), the manufactured right-hand side.  The reference of a case is computed once and shared
  per solve  u bit for bit, the history within 1e-12, the same count (under the margin rule of tests/test_gmres_solve_gpu.py, through
             rbgs_reference.compare)
  paths      fuse = 0 against the default and graph = 0 against the default: identical u (and count); reset + solve repeats the bits
  rhs        set_rhs with rhs_cases "uniform" and "spikes" on a live solver: the reference's u
  driver     mgpoisson -pc_type rbgs at npts 65 reproduces the Python solve's count
  refusals   what the smoother is not built for, at creation and on a live handle, each by its message"""
import os
import re
import subprocess

import numpy as np
import pytest

import rbgs_reference as RB
import rhs_cases
from oracle import Oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(npts, mesh, scale, v0, v1, "manufactured") for npts in (17, 65, 129, 513) for mesh in (0, 1, 2) for scale in (1.0, 0.8)
         for v0, v1 in ((1, 1), (2, 2), (3, 2))]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _solver(case, **kw):
    from multigrid_petsc_amd.solver import Solver
    npts, mesh, scale, v0, v1, rhs = case
    s = Solver(2, npts, RB.LEVELS[npts], v=(v0, v1), maxiter=100, scale=scale, mesh=mesh, pc_type="rbgs", **kw)
    if rhs == "manufactured":
        s.set_rhs_problem()
    else:
        s.set_rhs(RB.case_rhs(RB.hierarchy(Oracle(), npts, mesh), rhs))
    return s


@pytest.mark.parametrize("case", CASES, ids=[RB.case_key(c) for c in CASES])
def test_rbgs_solve_equals_the_reference(orc, case):
    ref = RB.reference(orc, case)
    s = _solver(case)
    it = s.solve()
    rn, u, bn = s.rnorm, s.solution(), s.bnorm
    m = min(len(rn), len(ref["rnorm"]))
    print(f"{RB.case_key(case)}: {it} cycles (reference {ref['iters']}), max relative history diff = "
          f"{(np.abs(rn[:m] - ref['rnorm'][:m]) / ref['rnorm'][:m]).max():.2e}, u differs in {int(np.sum(u != ref['u']))} of {u.size}")
    RB.compare(ref, it, rn, u, bn)
    s.close()


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in (65, 513) and c[2] == 1.0 and c[1] in (0, 2)], ids=RB.case_key)
def test_fuse_and_graph_change_no_bit_of_u(case):
    s = _solver(case)
    it = s.solve()
    rn, u = s.rnorm, s.solution()
    s.reset()                                        # again on the same solver: the recorded coarse-level graph is replayed from fresh state
    assert s.solve() == it and np.array_equal(s.rnorm, rn) and np.array_equal(s.solution(), u), "reset + solve"
    s.close()
    t = _solver(case, graph=0)
    assert t.solve() == it and np.array_equal(t.rnorm, rn) and np.array_equal(t.solution(), u), "graph=0"
    t.close()
    t = _solver(case, fuse=0)
    itf, rnf, uf = t.solve(), t.rnorm, t.solution()
    t.close()
    assert itf == it and np.array_equal(uf, u), "fuse=0"
    assert np.abs(rnf / rn - 1).max() <= 1e-12       # (the norm is summed by another kernel)
    t = _solver(case, fuse=2)                        # bit 1 alone: the prolongation pass without the fused residual passes
    assert t.solve() == it and np.array_equal(t.solution(), u), "fuse=2"
    t.close()


@pytest.mark.parametrize("family", rhs_cases.FAMILIES)
def test_set_rhs_on_a_live_solver(orc, family):
    """a manufactured solve first, then an arbitrary right-hand side on the same handle (its graph already recorded): the reference's u"""
    for npts, mesh, v in ((65, 0, (2, 2)), (129, 1, (3, 2))):
        s = _solver((npts, mesh, 1.0, v[0], v[1], "manufactured"))
        s.solve()
        seed = 5
        case = (npts, mesh, 1.0, v[0], v[1], ("rough" if family == "uniform" else family) + f":{seed}")
        ref = RB.reference(orc, case)
        s.set_rhs(rhs_cases.make(family, 2, npts, seed))
        s.reset()
        it = s.solve()
        RB.compare(ref, it, s.rnorm, s.solution(), s.bnorm)
        s.close()


def test_own_driver_takes_pc_type_rbgs(tmp_path):
    exe = os.path.join(ROOT, "multigrid_petsc_amd", "mgpoisson")
    case = (65, 0, 1.0, 2, 2, "manufactured")
    s = _solver(case)
    it = s.solve()
    rel = s.rnorm[-1] / s.rnorm[0]
    s.close()
    p = subprocess.run([exe, "-dim", "2", "-npts", "65", "-levels", "6", "-pc_type", "rbgs", "-ksp_richardson_scale", "1", "-iter", "100", "-v", "2,2",
                        "-write_fields", "0"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:]
    assert int(re.search(r"Number of iterations:\s+(\d+)", p.stdout).group(1)) == it
    assert abs(float(re.search(r"Relative residual = (\S+)", p.stdout).group(1)) - rel) <= 1e-12 * rel


def test_what_the_smoother_is_not_built_for_is_refused():
    from multigrid_petsc_amd.solver import MgError, Solver
    for kw, msg in ((dict(dim=3, npts=17, levels=3), "built for 2-D"),
                    (dict(dim=2, npts=17, levels=3, precision="mixed"), "not mixed precision"),
                    (dict(dim=2, npts=17, levels=3, ksp_type="chebyshev", eigenvalues=(0.2, 2.0)), "not Chebyshev"),
                    (dict(dim=2, npts=17, levels=3, nranks=2), "one GPU"),
                    (dict(dim=2, npts=17, levels=3, line_chunk=4), "must be 0 with pc_type rbgs"),
                    (dict(dim=2, npts=33, levels=3, xline_chunk=16), "must be 0 with pc_type rbgs"),
                    (dict(dim=2, npts=17, levels=3, line_tail=1), "must be 0 with pc_type rbgs")):
        with pytest.raises(MgError, match=msg):
            Solver(v=(2, 2), maxiter=20, scale=1.0, pc_type="rbgs", **kw)
    with pytest.raises(KeyError):
        Solver(2, 17, 3, pc_type="sor")
    s = _solver((17, 0, 1.0, 2, 2, "manufactured"))
    it = s.solve()
    u = s.solution()
    for call, name in ((lambda: s.fmg(1), "mg_solver_fmg"), (lambda: s.solve_fmg(1), "mg_solver_fmg"), (lambda: s.solve_gmres(30), "mg_solver_solve_gmres")):
        with pytest.raises(MgError, match=name + ".*not the red-black Gauss-Seidel smoother"):
            call()
    s.reset()                                        # the refusals leave the solver usable
    assert s.solve() == it == 6 and np.array_equal(s.solution(), u)
    assert s.tail_level == 0
    s.close()
