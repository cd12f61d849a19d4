"""Whole-cycle parity on ARBITRARY right-hand sides: Solver.set_rhs (mg_solver_set_rhs_host) against the CPU oracle's V-cycle on the same b
(Oracle.vcycle(b=), vcycle_mixed(b=), FmgRef(b0=)).

Every other whole-cycle test solves the manufactured problem, whose right-hand side is a discrete eigenvector of the operator, the sweep and
both transfers: each field of each cycle is one smooth single-signed mode, and what mg_solver.c composes -- which buffer, which ghost plane,
which pass, at which size -- never meets a sign change, a zero or a rough neighbourhood.  Here b is rough (uniform in (-1, 1)) or sparse (a
handful of +-1 spikes at positions no symmetry of the grid maps onto each other; tests/rhs_cases.py).

Bars (the project's own): u bit for bit, iteration count equal, ||b|| and the residual history to 1e-12 relative; slab ranks against one rank
to 1e-13 on the norms; a live solver given a new right-hand side against a fresh solver: everything bit for bit, norms included.  Before a
count of solve() is compared, the oracle's own history is shown to have no norm within (1 +- 1e-6) rtol ||b|| (rhs_cases.assert_stop_rule_clear):
the 1e-12 between two orders of summation then cannot decide the count."""
import time

import numpy as np
import pytest

import rhs_cases
from fmg_reference import FmgRef
from oracle import Oracle

pytestmark = pytest.mark.gpu
RTOL = 1e-12
EIG = (0.2, 2.0)
DEFAULT = 63 | 0xFF00                         # fuse bits 0-5 and 8-15: what fuse = -1 stands for
FAMILIES = rhs_cases.FAMILIES


class _Timed:
    """the oracle with the wall time of its calls added up (reported when the module is done: it is what bounds the large cases)"""

    def __init__(self, orc):
        self._orc, self.seconds = orc, 0.0
        self.L = orc.L

    def __getattr__(self, name):
        f = getattr(self._orc, name)
        if not callable(f):
            return f

        def timed(*a, **kw):
            t0 = time.perf_counter()
            try:
                return f(*a, **kw)
            finally:
                self.seconds += time.perf_counter() - t0
        return timed


@pytest.fixture(scope="module")
def orc():
    o = _Timed(Oracle())
    t0 = time.perf_counter()
    yield o
    print(f"\ntest_rhs_cycle_gpu: {time.perf_counter() - t0:.1f} s wall, {o.seconds:.1f} s of it inside the CPU oracle")


def _scale(dim):
    return 0.8 if dim == 2 else 6.0 / 7.0


def _depth(npts):
    return (npts - 1).bit_length() - 1


_B, _REF = {}, {}


def _b(family, dim, npts, salt=0, cuts=()):
    """the right-hand side of a case (kept while the module runs: the fields of the large cases take seconds to draw)"""
    key = (family, dim, npts, salt, tuple(cuts))
    if key not in _B:
        if npts > 600 and dim == 3:
            return rhs_cases.make(family, dim, npts, 7000 + 10 * npts + salt, cuts)      # (8 GiB at 1023^3: not kept)
        _B[key] = rhs_cases.make(family, dim, npts, 7000 + 10 * npts + salt, cuts)
    return _B[key]


def _ref(orc, b, tag, dim, npts, levels, v=(3, 3), cheb=False, mesh=0, mixed=False, maxiter=100, fixed=0):
    """the oracle on b (one run per case and module: the fuse ladder, the slabs and the replacement tests meet the same case again)"""
    key = (tag, dim, npts, levels, v, cheb, mesh, mixed, maxiter, fixed)
    if key not in _REF:
        if mixed:
            r = orc.vcycle_mixed(npts, levels, v[0], v[1], maxiter=max(maxiter, fixed), scale=_scale(3), fixed_cycles=fixed, b=b)
        else:
            kw = dict(ksp_type=1, emin=EIG[0], emax=EIG[1]) if cheb else dict(scale=_scale(dim))
            r = orc.vcycle(dim, npts, levels, v[0], v[1], maxiter=max(maxiter, fixed), use_csr=1 if mesh else 0, mesh=mesh, fixed_cycles=fixed, b=b, **kw)
        if not fixed:
            rhs_cases.assert_stop_rule_clear(r)
        if npts > 600 and dim == 3:
            return r
        _REF[key] = r
    return _REF[key]


def _solver(dim, npts, levels, v=(3, 3), cheb=False, maxiter=100, **kw):
    from multigrid_petsc_amd.solver import Solver
    if cheb:
        return Solver(dim, npts, levels, v=v, maxiter=maxiter, ksp_type="chebyshev", eigenvalues=EIG, **kw)
    return Solver(dim, npts, levels, v=v, maxiter=maxiter, scale=_scale(dim), **kw)


def _state(s):
    return s.iterations, s.bnorm, s.rnorm.copy(), s.solution()


def _same_as_oracle(st, ref, what=""):
    it, bn, rn, u = st
    dn = np.abs(rn / ref["rnorm"] - 1).max() if rn.shape == ref["rnorm"].shape else np.inf
    print(f"{what}: iterations {it} / {ref['iters']}, ||b|| rel diff {abs(bn / ref['bnorm'] - 1):.2e}, history max rel diff {dn:.2e}, "
          f"max|du| {np.abs(u - ref['u']).max():.2e}")
    assert it == ref["iters"], (it, ref["iters"])
    assert abs(bn - ref["bnorm"]) <= RTOL * ref["bnorm"]
    assert rn.shape == ref["rnorm"].shape and dn <= RTOL, f"residual history differs: max rel {dn}"
    assert np.array_equal(u, ref["u"]), f"solution not bit-identical, max diff {np.abs(u - ref['u']).max()}"


def _same_bits(a, b, what=""):
    assert a[0] == b[0] and a[1] == b[1], (what, a[0], b[0], a[1], b[1])
    assert np.array_equal(a[2], b[2]), f"{what}: the histories differ by {np.abs(a[2] / b[2] - 1).max()}"
    assert np.array_equal(a[3], b[3]), f"{what}: the fields differ by {np.abs(a[3] - b[3]).max()}"


def _same_fields(a, b, tol, what=""):
    """two cycles that differ in which kernels form the norms: the same u bits, the same count, the histories to tol"""
    assert a[0] == b[0], (what, a[0], b[0])
    assert abs(a[1] - b[1]) <= tol * b[1] and np.abs(a[2] / b[2] - 1).max() <= tol, what
    assert np.array_equal(a[3], b[3]), f"{what}: the fields differ by {np.abs(a[3] - b[3]).max()}"


def _host_mem_gib():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / 2 ** 20
    except OSError:
        pass
    return 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 Richardson, full depth
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dim,npts", [(2, 129), (2, 1025), (2, 2049), (2, 4097), (3, 33), (3, 65), (3, 129), (3, 257)])
def test_full_depth_solve_equals_the_oracle(orc, family, dim, npts):
    """2-D 1025 .. 4097: the three-sweep passes, the LDS tail and the coarse-level graph; 3-D: the two-sweep passes, the tail, the graph"""
    levels = _depth(npts)
    b = _b(family, dim, npts)
    ref = _ref(orc, b, family, dim, npts, levels)
    s = _solver(dim, npts, levels)
    s.set_rhs(b)
    s.solve()
    _same_as_oracle(_state(s), ref, f"{dim}-D {npts} {family}")
    s.close()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("family", FAMILIES)
def test_513_cubed_over_three_cycles_equals_the_oracle(orc, family):
    """fuse bits 10, 11 and 12 (the two-sweep norm pass, the sweep inside the restriction, prolongation + two sweeps) run from 255^3 up"""
    b = _b(family, 3, 513)
    ref = _ref(orc, b, family, 3, 513, 9, fixed=3)
    s = _solver(3, 513, 9)
    s.set_rhs(b)
    s.cycles(3)
    s.sync()
    _same_as_oracle(_state(s), ref, f"3-D 513 {family}")
    s.close()


@pytest.mark.timeout(3000)
@pytest.mark.parametrize("family", FAMILIES)
def test_headline_size_over_two_cycles_equals_the_oracle(orc, family):
    """1025^3, the headline grid, where the host has the memory for b, the oracle's seven fields and two copies of u"""
    need, have = 110.0, _host_mem_gib()
    if have < need:
        pytest.skip(f"the oracle's cycle at 1023^3 next to b and u needs ~{need:.0f} GiB of host memory, {have:.0f} GiB available")
    b = _b(family, 3, 1025)
    s = _solver(3, 1025, 10)
    s.set_rhs(b)
    s.cycles(2)
    s.sync()
    st = _state(s)
    s.close()
    _same_as_oracle(st, _ref(orc, b, family, 3, 1025, 10, fixed=2), f"3-D 1025 {family}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the fuse ladder on a random b
# ---------------------------------------------------------------------------------------------------------------------------------
LADDER = [DEFAULT & ~(1 << q) for q in (1, 2, 3, 5, 8, 9, 10, 11, 12, 13, 15)] + [0]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("dim,npts", [(2, 1025), (3, 129)])
def test_fuse_ladder_on_a_random_right_hand_side(orc, dim, npts):
    """the default mask against each of bits 1, 2, 3, 5, 8, 9, 10, 11, 12, 13, 15 cleared and against the kernel-per-operation cycle: the same u
    bits, the histories to 1e-12; the default one equals the oracle"""
    levels = _depth(npts)
    b = _b("uniform", dim, npts)
    ref = _ref(orc, b, "uniform", dim, npts, levels)
    out = {}
    for fuse in [DEFAULT] + LADDER:
        s = _solver(dim, npts, levels, fuse=fuse)
        s.set_rhs(b)
        s.solve()
        out[fuse] = _state(s)
        s.close()
    _same_as_oracle(out[DEFAULT], ref, f"{dim}-D {npts} default mask")
    for fuse in LADDER:
        _same_fields(out[fuse], out[DEFAULT], RTOL, f"fuse = {fuse:#x}")


@pytest.mark.timeout(900)
def test_fuse_ladder_at_513_cubed(orc):
    """bits 10, 11 and 12 where their passes run (from 255^3 up): three cycles on a random b with each of them cleared, and with all three"""
    b = _b("uniform", 3, 513)
    out = {}
    for fuse in (DEFAULT, DEFAULT & ~1024, DEFAULT & ~2048, DEFAULT & ~4096, DEFAULT & ~(1024 | 2048 | 4096)):
        s = _solver(3, 513, 9, fuse=fuse)
        s.set_rhs(b)
        s.cycles(3)
        s.sync()
        out[fuse] = _state(s)
        s.close()
    _same_as_oracle(out[DEFAULT], _ref(orc, b, "uniform", 3, 513, 9, fixed=3), "3-D 513 default mask")
    for fuse, st in out.items():
        _same_fields(st, out[DEFAULT], RTOL, f"fuse = {fuse:#x}")


# ---------------------------------------------------------------------------------------------------------------------------------
# Chebyshev
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("v", [(3, 3), (3, 1), (2, 2)])
@pytest.mark.parametrize("dim,npts", [(2, 257), (2, 1025), (2, 4097), (3, 65)])
def test_chebyshev_fused_and_step_by_step_equal_the_oracle(orc, family, v, dim, npts):
    """fuse bit 15 on (three-step passes, the Chebyshev tail, the graph) and off (every step a launch), both against the oracle's recurrence"""
    levels = _depth(npts)
    b = _b(family, dim, npts)
    ref = _ref(orc, b, family, dim, npts, levels, v=v, cheb=True, maxiter=200)
    for fuse in (-1, DEFAULT & ~32768):
        s = _solver(dim, npts, levels, v=v, cheb=True, maxiter=200, fuse=fuse)
        s.set_rhs(b)
        s.solve()
        _same_as_oracle(_state(s), ref, f"Chebyshev {dim}-D {npts} v={v} {family} fuse={fuse}")
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# stretched meshes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cheb", [False, True])
@pytest.mark.parametrize("npts", [129, 257])
@pytest.mark.parametrize("mesh", [1, 2])
def test_stretched_meshes_equal_the_assembled_leg(orc, family, cheb, npts, mesh):
    levels = _depth(npts)
    b = _b(family, 2, npts)
    ref = _ref(orc, b, family, 2, npts, levels, cheb=cheb, mesh=mesh, maxiter=1000)
    s = _solver(2, npts, levels, cheb=cheb, maxiter=1000, mesh=mesh)
    s.set_rhs(b)
    s.solve()
    assert ref["iters"] < 1000
    _same_as_oracle(_state(s), ref, f"mesh {mesh} {npts} {'Chebyshev' if cheb else 'Richardson'} {family}")
    s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# mixed precision
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("npts", [65, 129, 257])
def test_mixed_precision_equals_the_oracle(orc, family, npts):
    levels = _depth(npts)
    b = _b(family, 3, npts)
    ref = _ref(orc, b, family, 3, npts, levels, mixed=True)
    s = _solver(3, npts, levels, precision="mixed")
    s.set_rhs(b)
    s.solve()
    _same_as_oracle(_state(s), ref, f"mixed 3-D {npts} {family}")
    s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# full multigrid
# ---------------------------------------------------------------------------------------------------------------------------------
def _fmg_refs(orc, b, dim, npts, levels, k=3, maxiter=100, rtol=1e-7):
    """FmgRef(b0 = b) once per case: FMG(1), then V-cycles under the stop rule -- (u0, its two norms), (u after k cycles, k + 2 norms),
    (iterations, u, history) of solve_fmg.  fmg_then_cycles and solve_fmg of tests/fmg_reference.py are prefixes of this one run."""
    f = FmgRef(orc, dim, npts, levels, (3, 3), _scale(dim), b0=b)
    bnorm = f.bnorm()
    u = f.fmg(1)
    rn = [f.rnorm_of(f.zeros(0)), f.rnorm_of(u)]
    u0, uk, it = u, None, 1
    while it < maxiter and 100000000 * bnorm > rn[-1] and rn[-1] > rtol * bnorm:
        u = f.vcycle(0, b, u)
        rn.append(f.rnorm_of(u))
        it += 1
        if it == k + 1:
            uk = u
    assert it >= k + 1, "the case converges before the k cycles the test continues with"
    rn = np.array(rn)
    rhs_cases.assert_stop_rule_clear({"rnorm": rn[1:], "bnorm": bnorm, "iters": it})
    return dict(bnorm=bnorm, u0=u0, rn0=rn[:2], uk=uk, rnk=rn[:k + 2], it=it, u=u, rn=rn)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dim,npts", [(2, 1025), (2, 4097), (3, 129), (3, 513)])
def test_fmg_solve_fmg_and_fmg_then_cycles_equal_the_restatement(orc, family, dim, npts):
    levels, k = _depth(npts), 3
    b = _b(family, dim, npts)
    r = _fmg_refs(orc, b, dim, npts, levels, k)
    s = _solver(dim, npts, levels)
    s.set_rhs(b)
    assert s.fmg(1) == 1
    _same_as_oracle(_state(s), dict(iters=1, bnorm=r["bnorm"], rnorm=r["rn0"], u=r["u0"]), f"fmg {dim}-D {npts} {family}")
    s.cycles(k)
    s.sync()
    _same_as_oracle(_state(s), dict(iters=k + 1, bnorm=r["bnorm"], rnorm=r["rnk"], u=r["uk"]), f"fmg + {k} cycles {dim}-D {npts} {family}")
    s.set_rhs(b)
    s.solve_fmg(1)
    _same_as_oracle(_state(s), dict(iters=r["it"], bnorm=r["bnorm"], rnorm=r["rn"], u=r["u"]), f"solve_fmg {dim}-D {npts} {family}")
    s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# slabs on loopback ranks
# ---------------------------------------------------------------------------------------------------------------------------------
def _ranks(P, fn):
    from multigrid_petsc_amd.comm import LoopbackWorld
    world = LoopbackWorld(P)
    try:
        return world.run(fn)
    finally:
        world.close()


def _cuts(P, npts, levels, dist_min_n, **kw):
    """the first planes of the slabs of ranks 1 .. P-1 on the fine level, and every rank's (z0, nz)"""
    def fn(rank, comm):
        s = _solver(3, npts, levels, rank=rank, nranks=P, comm=comm, dist_min_n=dist_min_n, **kw)
        p = s.level_planes(0)
        s.close()
        return p
    planes = _ranks(P, fn)
    n = npts - 2
    assert planes[0][0] == 0 and sum(p[1] for p in planes) == n and all(planes[r][0] == planes[r - 1][0] + planes[r - 1][1] for r in range(1, P))
    return [p[0] for p in planes[1:]]


def _slab_run(P, npts, levels, dist_min_n, bs, ops, **kw):
    """every rank loads ITS planes [z0, z0 + nz) of each global right-hand side of bs in turn into one solver object and runs ops(s) on it:
    [[state per right-hand side] per rank].  b = None stands for the manufactured right-hand side."""
    n = npts - 2

    def fn(rank, comm):
        s = _solver(3, npts, levels, rank=rank, nranks=P, comm=comm, dist_min_n=dist_min_n, **kw)
        z0, nz = s.level_planes(0)
        out = []
        for b in bs:
            if b is None:
                s.set_rhs_problem()
            else:
                s.set_rhs(b.reshape(n, n * n)[z0:z0 + nz])
            ops(s)
            out.append(_state(s))
        s.close()
        return out
    return _ranks(P, fn)


def _joined(res, q):
    """the ranks' q-th results as one: (iterations, ||b||, history) of rank 0 after checking that every rank reports the same, u concatenated"""
    for r in res[1:]:
        assert r[q][0] == res[0][q][0] and r[q][1] == res[0][q][1] and np.array_equal(r[q][2], res[0][q][2])
    return res[0][q][0], res[0][q][1], res[0][q][2], np.concatenate([r[q][3] for r in res])


def _solve(s):
    s.solve()


SLABS = [(2, 33, 4, 15), (3, 65, 5, 15), (4, 65, 6, 31), (8, 129, 6, 31), (2, 65, 3, 15)]       # test_multirank_gpu.py: test_slab_ranks_equal_single_rank


@pytest.mark.timeout(900)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", ["fp64", "mixed", "chebyshev"])
@pytest.mark.parametrize("P,npts,levels,dist_min_n", SLABS)
def test_slab_ranks_on_their_slices_equal_one_rank_and_the_oracle(orc, family, kind, P, npts, levels, dist_min_n):
    """each rank calls set_rhs on its slice of the global b (a wrong z0 or plane count moves a spike to another plane): the concatenated u
    equals the one-rank result and the oracle bit for bit, with the halo exchange overlapped and blocking"""
    kw = dict(precision="mixed") if kind == "mixed" else dict(cheb=True) if kind == "chebyshev" else {}
    b = _b(family, 3, npts, salt=P, cuts=_cuts(P, npts, levels, dist_min_n, **kw) if family == "spikes" else ())
    ref = _ref(orc, b, (family, P), 3, npts, levels, cheb=kind == "chebyshev", mixed=kind == "mixed", maxiter=60)
    s = _solver(3, npts, levels, maxiter=60, **kw)
    s.set_rhs(b)
    s.solve()
    one = _state(s)
    s.close()
    _same_as_oracle(one, ref, f"one rank {npts} {kind} {family}")
    for overlap in (1, 0):
        st = _joined(_slab_run(P, npts, levels, dist_min_n, [b], _solve, maxiter=60, overlap=overlap, **kw), 0)
        _same_fields(st, one, 1e-13, f"P = {P}, overlap = {overlap}")
        _same_as_oracle(st, ref, f"P = {P} {npts} {kind} {family} overlap = {overlap}")


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("family", FAMILIES)
def test_four_slabs_at_513_equal_one_rank_and_the_oracle(orc, family):
    """513 wide, P = 4: the 91-byte fine level on slabs (fuse bit 14: prolongation + two sweeps, the mid-iterate norm, the owed sweep) over three cycles"""
    def ops(s):
        s.cycles(3)
        s.sync()
    b = _b(family, 3, 513, cuts=_cuts(4, 513, 9, 0) if family == "spikes" else ())
    # (uniform: the right-hand side and the oracle run of test_513_cubed_over_three_cycles_equals_the_oracle; the spikes sit at these cuts)
    ref = _ref(orc, b, (family, "four slabs") if family == "spikes" else family, 3, 513, 9, fixed=3)
    st = _joined(_slab_run(4, 513, 9, 0, [b], ops), 0)
    _same_as_oracle(st, ref, f"P = 4, 513 {family}")


# ---------------------------------------------------------------------------------------------------------------------------------
# replacing the right-hand side on a live solver
# ---------------------------------------------------------------------------------------------------------------------------------
# What mg_solver.c keeps "once per right-hand side" -- the neighbours' b ghost planes and far planes on slabs, pre_done / spec_valid / sweep_owed /
# iterate_behind, the recorded coarse-level graph, FMG's restricted b_l -- is invalidated in start(); a solver that reloads the SAME b (every other
# "second solve" test) cannot tell whether it is.
def _cyc(k):
    def ops(s):
        s.cycles(k)
        s.sync()
    return ops


def _fmg1(s):
    s.fmg(1)


def _solve_fmg(s):
    s.solve_fmg(1)


K = 4
# (name, first right-hand side: family or None = the manufactured one, what runs on it, second right-hand side, what runs on it, fixed count of the second)
SEQUENCES = [
    ("solve, set_rhs, solve", "first", _solve, "second", _solve, 0),
    ("cycles, set_rhs, cycles", "first", _cyc(K), "second", _cyc(K), K),
    ("solve, set_rhs, cycles", "first", _solve, "second", _cyc(K), K),
    ("set_rhs_problem, set_rhs, solve", None, _solve, "second", _solve, 0),
    ("set_rhs, set_rhs_problem, solve", "first", _solve, None, _solve, 0),
]


def _pair(family, dim, npts, cuts=()):
    """b1 of the other family than b2, b2 of `family`"""
    other = FAMILIES[1 - FAMILIES.index(family)]
    return _b(other, dim, npts, salt=1, cuts=cuts if other == "spikes" else ()), _b(family, dim, npts, salt=2, cuts=cuts if family == "spikes" else ())


def _ref_second(orc, b2, family, dim, npts, levels, fixed, maxiter=100):
    if b2 is None:
        return orc.vcycle(dim, npts, levels, 3, 3, maxiter=max(maxiter, fixed), scale=_scale(dim), fixed_cycles=fixed)
    return _ref(orc, b2, (family, "second"), dim, npts, levels, fixed=fixed, maxiter=maxiter)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,first,ops1,second,ops2,fixed", SEQUENCES, ids=[q[0].replace(", ", "-") for q in SEQUENCES])
@pytest.mark.parametrize("dim,npts", [(2, 2049), (3, 129)])
def test_a_new_right_hand_side_on_a_live_solver_one_rank(orc, family, name, first, ops1, second, ops2, fixed, dim, npts):
    """graph recorded at these sizes; the second result equals a fresh solver's on the second right-hand side bit for bit, norms included, and the oracle's"""
    levels = _depth(npts)
    b1, b2 = _pair(family, dim, npts)
    b1, b2 = (b1 if first else None), (b2 if second else None)
    ref = _ref_second(orc, b2, family, dim, npts, levels, fixed)
    if not fixed and b2 is None:
        rhs_cases.assert_stop_rule_clear(ref)
    out = []
    for bs in ([b1, b2], [b2]):
        s = _solver(dim, npts, levels)
        for b, ops in zip(bs, (ops1, ops2) if len(bs) == 2 else (ops2,)):
            if b is None:
                s.set_rhs_problem()
            else:
                s.set_rhs(b)
            ops(s)
        out.append(_state(s))
        s.close()
    _same_bits(out[0], out[1], name + ": live against fresh")
    _same_as_oracle(out[0], ref, f"{name} {dim}-D {npts} {family}")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dim,npts", [(2, 2049), (3, 129)])
def test_a_new_right_hand_side_after_fmg_one_rank(orc, family, dim, npts):
    """fmg(b1), set_rhs(b2), solve_fmg: FMG's restricted right-hand sides b_l belong to b1"""
    levels = _depth(npts)
    b1, b2 = _pair(family, dim, npts)
    r = _fmg_refs(orc, b2, dim, npts, levels)
    out = []
    for first in (b1, None):
        s = _solver(dim, npts, levels)
        if first is not None:
            s.set_rhs(first)
            s.fmg(1)
        s.set_rhs(b2)
        s.solve_fmg(1)
        out.append(_state(s))
        s.close()
    _same_bits(out[0], out[1], "fmg, set_rhs, solve_fmg: live against fresh")
    _same_as_oracle(out[0], dict(iters=r["it"], bnorm=r["bnorm"], rnorm=r["rn"], u=r["u"]), f"fmg, set_rhs, solve_fmg {dim}-D {npts} {family}")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,first,ops1,second,ops2,fixed", SEQUENCES, ids=[q[0].replace(", ", "-") for q in SEQUENCES])
def test_a_new_right_hand_side_on_live_slab_solvers(orc, family, name, first, ops1, second, ops2, fixed):
    """P = 3 slabs with two-sweep passes on the distributed levels: the neighbours' b ghost planes and far planes (b_ghost_ok, bfar_ok) are caches of the
    right-hand side that was there first"""
    P, npts, levels, dmin = 3, 65, 5, 15
    kw = dict(pair_min_n=15)
    b1, b2 = _pair(family, 3, npts, cuts=_cuts(P, npts, levels, dmin, **kw))
    b1, b2 = (b1 if first else None), (b2 if second else None)
    ref = _ref_second(orc, b2, (family, "slab"), 3, npts, levels, fixed)
    if not fixed and b2 is None:
        rhs_cases.assert_stop_rule_clear(ref)
    n = npts - 2

    def fn_for(bs, opss):
        def fn(rank, comm):
            s = _solver(3, npts, levels, rank=rank, nranks=P, comm=comm, dist_min_n=dmin, **kw)
            z0, nz = s.level_planes(0)
            for b, ops in zip(bs, opss):
                if b is None:
                    s.set_rhs_problem()
                else:
                    s.set_rhs(b.reshape(n, n * n)[z0:z0 + nz])
                ops(s)
            st = _state(s)
            s.close()
            return [st]
        return fn
    live = _ranks(P, fn_for([b1, b2], [ops1, ops2]))
    fresh = _ranks(P, fn_for([b2], [ops2]))
    for r in range(P):
        _same_bits(live[r][0], fresh[r][0], f"{name}: rank {r}, live against fresh")
    _same_as_oracle(_joined(live, 0), ref, f"{name} P = 3 {family}")
