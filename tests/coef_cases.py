"""Non-symmetric stencil coefficients for the tests that pin the kernel ABI's promise of INDEPENDENT coefficients (include/mgk.h:
3-D {(k-1),(i-1),(j-1),C,(j+1),(i+1),(k+1)}, 2-D {(i-1),(j-1),C,(j+1),(i+1)}, products summed in that order), and a numpy float64
restatement of the stencil operations in that order.  The level stencils of the Poisson problem have equal off-diagonal entries: a
kernel that reads a4 where a2 belongs, a host-side loader that transposes two slots, or a tail kernel that takes another level's
constants computes the same bits under them.  Under the sets made here every such slip moves the result by O(1).

Plain helper module (no fixtures).  Test infrastructure only."""
import numpy as np

from oracle import Oracle

CENTRE = -8.0            # strictly diagonally dominant: the off-diagonal magnitudes sum to at most 6 * 1.25 = 7.5


def distinct_coef(rng, dim, per_level=None):
    """7 (3-D) or 5 (2-D) pairwise distinct coefficients in the ABI's order: off-diagonals uniform(0.5, 1.25) in magnitude with random
    signs, both signs present, centre -8.  per_level = L: a list of L such sets, all values different across the sets too."""
    if per_level is not None:
        sets = []
        while len(sets) < per_level:
            As = distinct_coef(rng, dim)
            off = np.concatenate([np.delete(a, a.size // 2) for a in sets] + [np.delete(As, As.size // 2)])
            if np.unique(off).size == off.size:
                sets.append(As)
        return sets
    m = 7 if dim == 3 else 5
    c = m // 2
    while True:
        As = rng.uniform(0.5, 1.25, m) * rng.choice([-1.0, 1.0], m)
        As[c] = CENTRE
        off = np.delete(As, c)
        if (off > 0).any() and (off < 0).any() and np.unique(As).size == m:
            return As


def distinct_row_tables(rng, n):
    """(ctab (n, 5), dtab (n,)) of a 2-D row-table operator: per grid row five distinct values {(i-1), W, C, E, (i+1)} with W != E,
    off-diagonals as in distinct_coef, centre -(sum |others|) * uniform(1.0, 1.2), dtab = 1 / centre"""
    ct = np.empty((n, 5))
    for i in range(n):
        while True:
            off = rng.uniform(0.5, 1.25, 4) * rng.choice([-1.0, 1.0], 4)
            if (off > 0).any() and (off < 0).any() and np.unique(off).size == 4:
                break
        ct[i, [0, 1, 3, 4]] = off
        ct[i, 2] = -np.abs(off).sum() * rng.uniform(1.0, 1.2)
    assert np.all(ct[:, 1] != ct[:, 3])
    return ct, 1.0 / ct[:, 2]


def dense_field(rng, *shape):
    """uniform(-1, 1) without exact zeros: the oracle skips the terms that fall outside the grid where the kernels add a * 0; with no
    zero in the data neither a partial sum nor a result is a signed zero, so both give the same bits"""
    x = rng.uniform(-1.0, 1.0, shape)
    while not np.all(x):
        x[x == 0.0] = rng.uniform(-1.0, 1.0, int((x == 0.0).sum()))
    return x


# ---- the canonical arithmetic in numpy float64: elementwise operations only (one rounding per multiply and per add, no FMA), the shifted
# arrays added in ascending column order.  Fields: (nz, ny, nx) in 3-D, (ny, nx) in 2-D; zlo / zhi: the (ny, nx) planes below / above a slab
def np_apply(As, x, zlo=None, zhi=None):
    As = np.asarray(As, dtype=np.float64)
    p = np.zeros(tuple(s + 2 for s in x.shape))
    p[(slice(1, -1),) * x.ndim] = x
    if x.ndim == 2:
        assert As.size == 5 and zlo is None and zhi is None
        t = As[0] * p[:-2, 1:-1]
        t = t + As[1] * p[1:-1, :-2]
        t = t + As[2] * p[1:-1, 1:-1]
        t = t + As[3] * p[1:-1, 2:]
        t = t + As[4] * p[2:, 1:-1]
        return t
    assert As.size == 7
    if zlo is not None:
        p[0, 1:-1, 1:-1] = zlo
    if zhi is not None:
        p[-1, 1:-1, 1:-1] = zhi
    t = As[0] * p[:-2, 1:-1, 1:-1]
    t = t + As[1] * p[1:-1, :-2, 1:-1]
    t = t + As[2] * p[1:-1, 1:-1, :-2]
    t = t + As[3] * p[1:-1, 1:-1, 1:-1]
    t = t + As[4] * p[1:-1, 1:-1, 2:]
    t = t + As[5] * p[1:-1, 2:, 1:-1]
    t = t + As[6] * p[2:, 1:-1, 1:-1]
    return t


def _dinv(As):
    return 1.0 / float(As[len(As) // 2])


def np_residual(As, b, u, zlo=None, zhi=None):
    return b - np_apply(As, u, zlo, zhi)


def np_sweep(As, scale, b, u, zlo=None, zhi=None):
    """unew = u + scale * ((b - A u) * dinv)"""
    return u + scale * (np_residual(As, b, u, zlo, zhi) * _dinv(As))


def np_sweep_zero(As, scale, b):
    """the sweep from the zero guess: scale * (b * dinv), u is not read"""
    return scale * (b * _dinv(As))


def np_cheby_step(As, b, pk, pkm1, ckm1, ck, cz, zlo=None, zhi=None):
    """pkp1 = (c_km1 * pkm1 + c_k * pk) + c_z * ((b - A pk) * dinv)"""
    return (ckm1 * pkm1 + ck * pk) + cz * (np_residual(As, b, pk, zlo, zhi) * _dinv(As))


class DistinctOracle(Oracle):
    """the CPU oracle with level_stencil() replaced: every (dim, npts, level) gets its own distinct_coef set (seeded by the triple, so
    a test, its helpers and a later run see the same one).  A test body that takes its coefficients from orc.level_stencil(...) runs
    on non-symmetric operators when it is handed this object -- fine and coarse level with different sets, 1 / centre following.
    `served` counts the sets handed out, so a caller can tell that a body really took its coefficients from here."""

    def __init__(self):
        super().__init__()
        self.served = 0

    def level_stencil(self, dim, npts, l):
        h = super().level_stencil(dim, npts, l)[1]
        self.served += 1
        return distinct_coef(np.random.default_rng([20261, dim, npts, l]), dim), h
