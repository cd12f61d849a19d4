"""The 75-byte 3-D fine level (fuse bit 16, MG_FUSE_TRIPLE_MID: (P + S1, S2)(S3, N + S1', S2')(S3' + R)) against the 91-byte one it replaces:
npts = 513 (511^3, 9 levels), V(3,3), fp64, scale 6/7.  The two cycles make the same sweeps in other passes: solution() is equal bit for bit and
the residual history to 1e-13 relative (the norm is the same sum of squares reduced over other partials) -- after a fixed number of cycles in two
calls, after a solve to 1e-7, after a solve stopped by maxiter (its last cycle is expected to be the last) and after one that stops where no last
cycle was expected (finalize_iterate materialises the iterate).  The profile counters show that
the new pass really runs: one three-sweep launch (kind 2) per cycle with the bit, none without."""
import numpy as np
import pytest

from multigrid_petsc_amd import FUSE_AUTO, FUSE_TRIPLE_MID, Fuse
from multigrid_petsc_amd.solver import Solver

pytestmark = pytest.mark.gpu

NPTS, LEVELS, SCALE = 513, 9, 6.0 / 7.0
ON, OFF = int(Fuse.DEFAULT) | FUSE_TRIPLE_MID, int(Fuse.DEFAULT) & ~FUSE_TRIPLE_MID
RTOL = 1e-13


def _run(fuse, what, **kw):
    s = Solver(3, NPTS, LEVELS, v=(3, 3), scale=SCALE, device=0, fuse=fuse, **kw)
    try:
        s.set_rhs_problem()
        s.profile(True)
        what(s)
        s.sync()
        return {"it": s.iterations, "rn": s.rnorm, "u": s.solution(), "triple": s.profile_read(2)[1], "pair": s.profile_read(1)[1]}
    finally:
        s.close()


def _same(on, off):
    assert on["it"] == off["it"]
    rel = np.abs(on["rn"] - off["rn"]) / off["rn"]
    print(f"iterations {on['it']}, max rel diff of the residual history {rel.max():.2e}, three-sweep launches {on['triple']} / {off['triple']}, "
          f"two-sweep launches {on['pair']} / {off['pair']}")
    assert rel.max() <= RTOL, rel
    assert np.array_equal(on["u"], off["u"]), f"{np.count_nonzero(on['u'] != off['u'])} unknowns differ, max {np.abs(on['u'] - off['u']).max()}"
    assert off["triple"] == 0


def test_cycles_in_two_calls():
    """cycles(3) then cycles(2): the second call starts from the state the first one left (two speculative sweeps in tmp, u one sweep behind)"""
    def what(s):
        s.cycles(3)
        s.cycles(2)
    on, off = _run(ON, what, maxiter=10), _run(OFF, what, maxiter=10)
    _same(on, off)
    assert on["it"] == 5
    # every cycle of a fixed count but the last one of each call (which the caller knows to be the last: no sweep is owed) takes the pass
    assert on["triple"] == 3, on["triple"]
    assert on["pair"] < off["pair"]
    auto = _run(-1, what, maxiter=10)
    assert auto["triple"] == on["triple"] and np.array_equal(auto["u"], on["u"]) and np.array_equal(auto["rn"], on["rn"])          # -1 selects the bit
    assert FUSE_AUTO == ON


def test_solve_to_tolerance():
    on, off = _run(ON, lambda s: s.solve(), maxiter=50, rtol=1e-7), _run(OFF, lambda s: s.solve(), maxiter=50, rtol=1e-7)
    _same(on, off)
    assert 3 <= on["it"] < 50 and on["rn"][-1] <= 1e-7 * on["rn"][0] * (1 + 1e-12) and on["triple"] >= 1


def test_solve_stopped_by_maxiter():
    """maxiter = 3 stops the iteration long before the tolerance.  The solve loop expects the third cycle to be the last (the count runs out): it
    owes no sweep; the two before it take the new pass"""
    on, off = _run(ON, lambda s: s.solve(), maxiter=3, rtol=1e-7), _run(OFF, lambda s: s.solve(), maxiter=3, rtol=1e-7)
    _same(on, off)
    assert on["it"] == 3 and on["rn"][-1] > 1e-7 * on["rn"][0] and on["triple"] == 2


def test_solve_stopped_where_no_last_cycle_was_expected():
    """rtol = 0.3: the first cycle already reaches it, and nothing told the loop so (no contraction is known before the first cycle): its norm
    pass was the new one, u is one sweep behind the iterate the norm belongs to, tmp two sweeps ahead, and finalize_iterate makes the one sweep"""
    on, off = _run(ON, lambda s: s.solve(), maxiter=50, rtol=0.3), _run(OFF, lambda s: s.solve(), maxiter=50, rtol=0.3)
    _same(on, off)
    assert on["it"] == 1 and on["triple"] == 1
