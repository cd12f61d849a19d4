"""GPU tier of the recorded reference output (tests/golden/ref_assembly.npz; reads tests/golden and nothing of the reference tree).

1. The reference's own b[0] against the device right-hand side.  mg_solver_set_rhs_problem builds b on the device (sin_tables on the host,
   mgk_fill_separable_f64 on the GPU); the recorded b[0] is what the reference handed to VecSetValue.  Two solvers, one fed by each, must
   agree in ||b||, the residual history and every bit of the iterate after two cycles; 63 and 127 unknowns per side lie on either side of a
   64-lane wave in the fill kernel.  The bit-level pin of the host tables is the CPU program (tests/ref_tables_dump.c); this is the only
   route from the recorded b to the device fill, and the sensitivity check shows that the probe resolves b to 2^-40 relative.
2. The chain reference -> oracle -> product at the recorded assembly shapes: tests/test_reference_fixtures_cpu.py pins the oracle's A, R, P and
   b to the recorded stream; here Solver.solve() must agree with the oracle's assembled leg on those operators as __graft_entry__.smoke()
   asks: iteration count, history within 1e-12 relative, solution bit for bit."""
import numpy as np
import pytest

import ref_fixtures as RF
from oracle import Oracle

pytestmark = pytest.mark.gpu
SCALE = 0.8
RECORDED_B = {17: (17, 3, 3, 2, 1), 33: (33, 4, 4, 2, 1), 65: (65, 1, 1, 2, 0), 129: (129, 1, 1, 2, 0)}      # where b[0] of npts is recorded
DEPTH = {17: 4, 33: 5, 65: 6, 129: 7}                                                                       # levels down to the 1 x 1 grid


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def asm():
    return RF.load_assembly()


def _two_cycles(npts, mesh, b=None):
    from multigrid_petsc_amd.solver import Solver
    s = Solver(2, npts, DEPTH[npts], mesh=mesh, scale=SCALE)
    if b is None:
        s.set_rhs_problem()
    else:
        s.set_rhs(b)
    s.cycles(2)
    out = (s.bnorm, s.rnorm, s.solution())
    s.close()
    return out


@pytest.mark.parametrize("npts", [17, 33, 65, 129])
@pytest.mark.parametrize("mesh", [0, 1, 2])
def test_device_right_hand_side_equals_the_recorded_one(asm, mesh, npts):
    b = RF.stream_vector(asm[(mesh,) + RECORDED_B[npts]], (npts - 2) ** 2)
    bn_a, rn_a, u_a = _two_cycles(npts, mesh)
    bn_b, rn_b, u_b = _two_cycles(npts, mesh, b)
    print(f"mesh {mesh} npts {npts}: bnorm {bn_a!r} / {bn_b!r}, rnorm {rn_a} / {rn_b}, differing solution entries {int(np.sum(u_a != u_b))}")
    assert rn_a.size == 3
    assert RF.same_bits(np.float64(bn_a), np.float64(bn_b))
    assert RF.same_bits(rn_a, rn_b)
    assert RF.same_bits(u_a, u_b)
    # sensitivity: one entry of the recorded b scaled by 1 + 2^-40 must show in the iterate
    moved = b.copy()
    q = ((npts - 2) // 2) * (npts - 2) + (npts - 2) // 3
    moved[q] = moved[q] * (1.0 + 2.0 ** -40)
    assert moved[q] != b[q]
    u_c = _two_cycles(npts, mesh, moved)[2]
    assert not np.array_equal(u_c, u_b)


@pytest.mark.parametrize("shape", [(9, 2), (17, 3), (33, 4)])
@pytest.mark.parametrize("mesh", [0, 1, 2])
def test_solve_equals_the_oracle_on_the_recorded_operators(orc, asm, mesh, shape):
    from multigrid_petsc_amd.solver import Solver
    npts, levels = shape
    assert (mesh, npts, levels, levels, 2, 1) in asm          # the shape whose A, R, P and b the CPU tier pins to the recording
    s = Solver(2, npts, levels, v=(3, 3), maxiter=1000, scale=SCALE, mesh=mesh)
    s.set_rhs_problem()
    it = s.solve()
    ref = orc.vcycle(2, npts, levels, 3, 3, maxiter=1000, scale=SCALE, use_csr=1, mesh=mesh)
    rel = np.abs(s.rnorm - ref["rnorm"]) / ref["rnorm"]
    print(f"mesh {mesh} npts {npts} levels {levels}: {it} / {ref['iters']} cycles, max rel diff of the history {rel.max():.2e}")
    assert it == ref["iters"]
    assert rel.max() <= 1e-12
    assert np.array_equal(s.solution(), ref["u"])
    s.close()
