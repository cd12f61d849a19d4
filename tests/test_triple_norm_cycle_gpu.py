"""The 66-byte 3-D fine level (fuse bit 17, MG_FUSE_TRIPLE_NORM; csrc/mg_solver.c triple_norm_ok(), mg_triple.c):
(P + S1, S2, S3)(N + S1', S2', S3')(R) against the 75-byte level of bit 16 alone, (P + S1, S2)(S3, N + S1', S2')(S3' + R), inside one build.

npts = 513: the smallest cube with rows of 512 (level 0 is 511 wide).  The right-hand side is a seeded random field.  The two masks make the
same sweeps in other passes: solution() is equal bit for bit.  The norms are sums of the same squared residuals over other partials (with
the bit, of the stored iterate per block of the stacked pass; without it, of the iterate the middle pass never stores): the residual
history is held to MID_RTOL of tests/test_triple_prolong_cycle_gpu.py, the figure of the whole-cycle A/B tests.

Three cases, and a fourth that stops a solve where no last cycle was expected:
  full depth (9 levels; the coarse-level graph starts at level 2, level 1 feeds it), cycles(3) then cycles(2): the norm + three-sweep pass runs
    in every cycle but the closing one of each call (3 launches), the prolongation + three-sweep pass on level 0 in all five;
  levels = 3 (511, 255, 127: too few coarse levels for a graph), the same two calls: the wiring applies, nothing is recorded;
  full depth, solve() to 1e-4: about four cycles.
The counters: Solver.triple_norm_launches > 0 with the bit and 0 without; Solver.graph_rerecorded 0; and the plain-sweep profile count
(kind 0: on level 0 of these runs only finalize_iterate()'s sweep is one) is 0 with the bit -- a solve that stops owes no sweep.
One more test holds the per-width default: fuse = -1 runs the pass at npts = 1025 and not at 513."""
import numpy as np
import pytest

from multigrid_petsc_amd import FUSE_TRIPLE_MID, FUSE_TRIPLE_NORM, Fuse
from multigrid_petsc_amd.solver import Solver
from test_triple_prolong_cycle_gpu import MID_RTOL

pytestmark = pytest.mark.gpu

NPTS, SCALE = 513, 6.0 / 7.0
OFF = int(Fuse.DEFAULT) | FUSE_TRIPLE_MID
ON = OFF | FUSE_TRIPLE_NORM


@pytest.fixture(scope="module")
def rhs():
    return np.random.default_rng(71000).uniform(-1.0, 1.0, (NPTS - 2) ** 3)


def _run(fuse, what, rhs, levels=9, **kw):
    s = Solver(3, NPTS, levels, v=(3, 3), scale=SCALE, device=0, fuse=fuse, **kw)
    try:
        s.set_rhs(rhs)
        s.profile(True)
        what(s)
        s.sync()
        return {"it": s.iterations, "rn": s.rnorm.copy(), "u": s.solution(), "norm": s.triple_norm_launches, "pro": s.prolong_triple_launches(0),
                "rerec": s.graph_rerecorded, "plain": s.profile_read(0)[1], "pair": s.profile_read(1)[1], "triple": s.profile_read(2)[1]}
    finally:
        s.close()


def _both(what, rhs, **kw):
    on, off = _run(ON, what, rhs, **kw), _run(OFF, what, rhs, **kw)
    rel = np.abs(on["rn"] - off["rn"]) / off["rn"]
    print(f"iterations {on['it']} / {off['it']}, max rel diff of the residual history {rel.max():.2e}; on / off: norm + three-sweep launches "
          f"{on['norm']} / {off['norm']}, prolongation + three-sweep launches on level 0 {on['pro']} / {off['pro']}, kind-2 launches {on['triple']} / "
          f"{off['triple']}, two-sweep launches {on['pair']} / {off['pair']}, plain sweeps {on['plain']} / {off['plain']}, re-recordings {on['rerec']} / {off['rerec']}")
    assert on["it"] == off["it"]
    assert rel.max() <= MID_RTOL, rel
    assert np.array_equal(on["u"], off["u"]), f"{np.count_nonzero(on['u'] != off['u'])} unknowns differ, max {np.abs(on['u'] - off['u']).max()}"
    assert on["norm"] > 0 and off["norm"] == 0
    assert on["triple"] == on["norm"]                   # timed as profile kind 2, and nothing else is with the bit on
    assert on["rerec"] == 0 and off["rerec"] == 0
    assert on["plain"] == 0 and on["plain"] <= off["plain"]
    return on, off


def _two_calls(s):
    s.cycles(3)
    s.cycles(2)


def test_cycles_in_two_calls(rhs):
    on, off = _both(_two_calls, rhs, maxiter=10)
    assert on["it"] == 5
    # every cycle but the closing one of each call evaluates its norm in the pass; every cycle post-smooths level 0 in the prolongation pass,
    # which bit 16 alone takes in the closing cycles only
    assert on["norm"] == 3 and on["pro"] == 5 and off["pro"] == 2, (on, off)
    # a call's first cycle has nothing to adopt (the zero guess; the closing cycle before it made no speculative sweeps) and keeps its pair
    assert on["pair"] == 1, on["pair"]


def test_shallow_hierarchy(rhs):
    on, off = _both(_two_calls, rhs, levels=3, maxiter=10)
    assert on["it"] == 5 and on["norm"] == 3 and on["pro"] == 5, on


def test_solve_to_tolerance(rhs):
    on, off = _both(lambda s: s.solve(), rhs, maxiter=50, rtol=1e-4)
    assert 2 <= on["it"] <= 8 and on["rn"][-1] <= 1e-4 * on["rn"][0] * (1 + 1e-12), (on["it"], on["rn"])


def test_the_default_mask_takes_the_bit_per_width():
    """fuse = -1: the bit is added where level 0 has rows of 1024 (the gate of profiles/triple_norm/README.md is met there), not at rows of 512"""
    for npts, levels, want in ((1025, 10, 1), (513, 9, 0)):
        s = Solver(3, npts, levels, v=(3, 3), scale=SCALE, device=0, maxiter=5)
        try:
            s.set_rhs_problem()
            s.cycles(2)
            s.sync()
            assert s.triple_norm_launches == want and s.prolong_triple_launches(0) == (2 if want else 1), (npts, s.triple_norm_launches)
        finally:
            s.close()


def test_solve_stopped_where_no_last_cycle_was_expected(rhs):
    """rtol = 0.3: the first cycle reaches it unannounced.  Without the bit u is one sweep behind the iterate and finalize_iterate() makes that
    sweep (one plain sweep in the profile); with it u is the iterate and nothing runs after the loop"""
    on, off = _both(lambda s: s.solve(), rhs, maxiter=50, rtol=0.3)
    assert on["it"] == 1 and on["norm"] == 1 and on["plain"] == 0 and off["plain"] == 1, (on["plain"], off["plain"])
