"""The prolongation + three-sweep pass in the cycle (fuse bit 16 in the generic branch of prolong_smooth(), csrc/mg_solver.c; mg_triple.c): where
the post-smoothing of a 511- / 1023-wide level was (P + S1)(S2, S3) it is one pass, (P + S1, S2, S3).  The switch is Tune.NO_PROLONG_TRIPLE on
against off inside one build, and bit 16 off as well.  The iterates are the same sweeps: solution() is equal bit for bit.  Against the
switch the residual history is equal exactly (the norm passes are the same launches on the same fields).  Against bit 16 off it is equal
exactly where the run made no launch of the bit's middle pass (profile kind 2: none with v = (4, 4) or without MG_FUSE_PROLONG_PAIR); where
it did, the norms of those cycles come from another kernel with other partial sums in both builds alike, and the history is held to the
1e-13 relative of tests/test_triple_mid_cycle_gpu.py, which compares the same two masks.  (Measured on an MI355X: against the switch 0 in
every case; against bit 16 off 1.47e-16 in cycles(3) + cycles(2) and in the solve to 1e-7, 0 in the other cases, whose norms either mask forms
in the same launches.  Exact equality against bit 16 off cannot hold there with or without this pass: the bit also switches the middle pass.)

npts = 513 (level 0 is 511 wide; the level below is too narrow and feeds the coarse-level graph): the pass runs on level 0 in the last cycle of
a call, which takes the generic branch; with v = (4, 4) or without MG_FUSE_PROLONG_PAIR every cycle takes it.  The launch counter
(Solver.prolong_triple_launches) shows that the pass ran, and that the switch kept it off.

npts = 1025: the smallest cube whose level 1 is 511 wide -- the pass runs there in every cycle, and on level 0 in the last cycle of a call.  The
residual history (every cycle's fine-level norm depends on level 1's post-smoothing) is compared there, and the counters; not the 8.6 GB solution."""
import numpy as np
import pytest

from multigrid_petsc_amd import FUSE_TRIPLE_MID, Fuse, Tune
from multigrid_petsc_amd.mgk import tuning
from multigrid_petsc_amd.solver import Solver

pytestmark = pytest.mark.gpu

SCALE = 6.0 / 7.0
ON, BIT_OFF = int(Fuse.DEFAULT) | FUSE_TRIPLE_MID, int(Fuse.DEFAULT) & ~FUSE_TRIPLE_MID
NO_PRO = int(Tune.NO_PROLONG_TRIPLE)
MID_RTOL = 1e-13


def _run(what, npts=513, levels=9, fuse=ON, variant=-1, v=(3, 3), solution=True, **kw):
    with tuning(variant, -1):
        s = Solver(3, npts, levels, v=v, scale=SCALE, device=0, fuse=fuse, **kw)
        try:
            s.set_rhs_problem()
            s.profile(True)
            what(s)
            s.sync()
            return {"it": s.iterations, "rn": s.rnorm.copy(), "u": s.solution() if solution else None,
                    "n": [s.prolong_triple_launches(l) for l in range(3)], "mid": s.profile_read(2)[1]}
        finally:
            s.close()


def _three(what, **kw):
    """(with the pass, with the switch, with bit 16 off), the last two held to the first"""
    fuse = kw.pop("fuse", ON)
    on, sw, off = _run(what, fuse=fuse, **kw), _run(what, fuse=fuse, variant=NO_PRO, **kw), _run(what, fuse=fuse & ~FUSE_TRIPLE_MID, **kw)
    print(f"iterations {on['it']}, launches per level: on {on['n']}, switch {sw['n']}, bit off {off['n']}; middle-pass launches {on['mid']} / {sw['mid']} / {off['mid']}")
    for name, other in (("switch", sw), ("bit 16 off", off)):
        assert other["n"] == [0, 0, 0], (name, other["n"])
        assert on["it"] == other["it"], name
        rel = np.abs(on["rn"] - other["rn"]) / other["rn"]
        print(f"{name}: max rel diff of the residual history {rel.max():.2e}")
        if name == "switch" or on["mid"] == 0:
            assert np.array_equal(on["rn"], other["rn"]), (name, on["rn"].tolist(), other["rn"].tolist())
        else:
            assert rel.max() <= MID_RTOL, (name, rel)
        if on["u"] is not None:
            assert np.array_equal(on["u"], other["u"]), f"{name}: {np.count_nonzero(on['u'] != other['u'])} unknowns differ"
    assert sw["mid"] == on["mid"] and off["mid"] == 0
    return on


def test_cycles_in_two_calls():
    """cycles(3) then cycles(2): the last cycle of each call takes the pass on level 0"""
    def what(s):
        s.cycles(3)
        s.cycles(2)
    on = _three(what, maxiter=10)
    assert on["it"] == 5 and on["n"] == [2, 0, 0], on["n"]


def test_solve_to_tolerance():
    on = _three(lambda s: s.solve(), maxiter=50, rtol=1e-7)
    assert 3 <= on["it"] < 50 and on["rn"][-1] <= 1e-7 * on["rn"][0] * (1 + 1e-12)
    print("launches", on["n"])


def test_solve_stopped_by_maxiter():
    """the solve loop expects the third cycle to be the last: it takes the generic branch, and with it the pass"""
    on = _three(lambda s: s.solve(), maxiter=3, rtol=1e-7)
    assert on["it"] == 3 and on["n"] == [1, 0, 0], on["n"]


def test_solve_stopped_where_no_last_cycle_was_expected():
    """rtol = 0.3: the first cycle reaches it unannounced; whatever branch it took, the three runs agree"""
    on = _three(lambda s: s.solve(), maxiter=50, rtol=0.3)
    assert on["it"] == 1
    print("launches", on["n"])


def test_four_sweeps_route_every_cycle_through_the_pass():
    """v = (4, 4): bit 12 wants v0 = 3, so every cycle's post-smoothing is the generic branch: the pass and one more sweep"""
    on = _three(lambda s: s.cycles(3), v=(4, 4), maxiter=10)
    assert on["it"] == 3 and on["n"] == [3, 0, 0], on["n"]


def test_without_the_prolongation_pair_every_cycle_takes_the_pass():
    on = _three(lambda s: s.cycles(3), fuse=ON & ~int(Fuse.PROLONG_PAIR), maxiter=10)
    assert on["it"] == 3 and on["n"] == [3, 0, 0], on["n"]


def test_level_one_of_1025():
    """cycles(2) then cycles(1): level 1 (511 wide, outside the coarse-level graph) takes the pass in all three cycles, level 0 in the last cycle
    of each call"""
    def what(s):
        s.cycles(2)
        s.cycles(1)
    on = _run(what, npts=1025, levels=10, solution=False, maxiter=10)
    assert on["it"] == 3 and on["n"] == [2, 3, 0], on["n"]
    sw = _run(what, npts=1025, levels=10, solution=False, variant=NO_PRO, maxiter=10)
    assert sw["n"] == [0, 0, 0] and np.array_equal(on["rn"], sw["rn"]), (on["rn"], sw["rn"])
