"""Right-hand sides for the whole-cycle parity tests: seeded, made with numpy alone (nothing here touches the oracle or the product).

The manufactured right-hand side of the reference (src/solver.c:558-620) is a discrete eigenvector of the operator, of the Jacobi sweep, of
full weighting and of interpolation at once: every field of every cycle is one smooth single-signed mode.  These two families are not:

  uniform   default_rng(seed).uniform(-1, 1, N): rough, mixed sign, every neighbour different
  spikes    zeros except a handful of +-1 entries -- next to a corner, on an edge row, on the last plane, on both planes next to every slab
            cut, a few interior ones -- no two of which are images of each other under the mirrors and axis swaps of the square / cube:
            a wrong neighbour, ghost plane or stale halo moves a spike's response by O(1), and no symmetry of the grid can hide it

Fields are compact lexicographic, index (k*n + i)*n + j (3-D), i*n + j (2-D), n = npts - 2 unknowns per side."""
import numpy as np

FAMILIES = ("uniform", "spikes")


def uniform(dim, npts, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (npts - 2) ** dim)


def _orbit(p, n):
    """invariant of the orbit of grid point p under the mirrors and axis permutations of the n^d grid"""
    return tuple(sorted(min(c, n - 1 - c) for c in p))


def spikes_min_npts(dim):
    """the smallest grid with enough orbits on its boundary for the spikes (2-D: the 7^2 grid has three edge orbits, four are needed)"""
    return 17 if dim == 2 else 9


def spike_positions(dim, npts, seed, cuts=()):
    """[(index tuple slowest axis first, sign)]; cuts: first planes of the slabs of ranks 1 .. P-1 (3-D)"""
    n = npts - 2
    if n < spikes_min_npts(dim) - 2:
        raise ValueError("spikes: the grid is too small for positions that are not images of each other")
    rng = np.random.default_rng(seed)
    taken, out = set(), []

    def put(fixed):
        """fixed: {axis: coordinate}; the other coordinates are drawn until the point's orbit is a new one"""
        for _ in range(10000):
            p = tuple(fixed[a] if a in fixed else int(rng.integers(1, n - 1)) for a in range(dim))
            if _orbit(p, n) not in taken:
                taken.add(_orbit(p, n))
                out.append((p, 1.0 if rng.integers(0, 2) else -1.0))
                return
        raise ValueError("spikes: no free orbit left")

    put({a: (1 if a == dim - 1 else 0) for a in range(dim)})          # next to the corner (0, .., 0, 1)
    put({a: 0 for a in range(dim - 1)})                               # on the edge row i = 0 (k = 0)
    put({0: n - 1})                                                   # on the last plane (3-D) / last row (2-D)
    put({dim - 1: n - 1})                                             # in the last column
    for z in cuts:                                                    # both planes next to every cut
        if not 0 < z < n:
            raise ValueError(f"spikes: cut {z} outside (0, {n})")
        put({0: z - 1})
        put({0: z})
    for _ in range(3):
        put({})
    return out


def spikes(dim, npts, seed, cuts=()):
    n = npts - 2
    b = np.zeros((n,) * dim)
    for p, sgn in spike_positions(dim, npts, seed, cuts):
        b[p] = sgn
    return b.ravel()


def make(family, dim, npts, seed, cuts=()):
    if family == "uniform":
        return uniform(dim, npts, seed)
    if family == "spikes":
        return spikes(dim, npts, seed, cuts)
    raise ValueError(family)


def stop_rule_clear(ref, rtol=1.0e-7):
    """on an ORACLE history: no norm of it -- the last two decide where the loop stops -- lies within (1 +- 1e-6) rtol ||b||"""
    q = np.asarray(ref["rnorm"]) / (rtol * ref["bnorm"])
    return bool(np.all(np.abs(q - 1.0) > 1e-6))


def assert_stop_rule_clear(ref, rtol=1.0e-7, maxiter=None):
    """The precondition of every comparison of solve(): on the oracle's own history the norms (the last two above all) lie outside
    (1 +- 1e-6) rtol ||b||, so an equal iteration count is not decided by the 1e-12 between two orders of summation.  A case that fails
    this gets another seed; it is never skipped."""
    q = np.asarray(ref["rnorm"]) / (rtol * ref["bnorm"])
    assert len(q) >= 2
    if maxiter is not None:
        assert ref["iters"] < maxiter and q[-1] < 1.0 < q[-2], "the oracle ran out of iterations"
    assert stop_rule_clear(ref, rtol), f"stop decision near a tie: rnorm[-2], rnorm[-1] = {q[-2]:.9f}, {q[-1]:.9f} x rtol ||b||"
