"""Red-black Gauss-Seidel in numpy: the definition that mgk_rbgs_2d_f64 / mgk_prolong_rbgs_2d_f64 (csrc/mgk_rbgs.hip), csrc/mg_rbgs.c and the
cycle of Solver(pc_type="rbgs") are held to, operation for operation.  Test infrastructure only.

Level field of ny x nx unknowns, row i with the coefficients {S, W, C, E, N}_i = ct[i, 0..4] and dinv_i (1 / C_i on the levels of a solver).
Point (i, j) -- 0-based interior row and column -- has the colour (i + j) & 1.  One sweep is two half-sweeps, colour 0 first, then colour 1;
a half-sweep of colour c replaces every point of colour c by

    u' = u + s ((b - t) dinv_i),    t = S u(i-1, j) + W u(i, j-1) + C u(i, j) + E u(i, j+1) + N u(i+1, j), summed in that order,

over the current field (ghosts are zeros), and passes the other points through.  From the zero guess: the same on a zeroed field.  Every
product and every sum is rounded on its own (numpy does not contract).  The cycle is the loop of oracle/mgo.c's mgo_vcycle with these
sweeps as the smoother, the row-table operator for A u, Oracle.restrict / Oracle.prolong_add for the transfers and Oracle.sumsq for the
norms; the row tables of a level come from the oracle's ASSEMBLED rows (line_reference.level_table), not from the product."""
import math

import numpy as np

import line_reference as LR


def colour(ny, nx):
    """(ny, nx) array of (i + j) & 1"""
    return (np.arange(ny)[:, None] + np.arange(nx)[None, :]) & 1


def apply(ct, u):
    """A u of the row-table operator on a rectangular field: the five terms in the order S, W, C, E, N"""
    ny, nx = u.shape
    p = np.zeros((ny + 2, nx + 2))
    p[1:-1, 1:-1] = u
    t = ct[:, 0:1] * p[:-2, 1:-1]
    t = t + ct[:, 1:2] * p[1:-1, :-2]
    t = t + ct[:, 2:3] * p[1:-1, 1:-1]
    t = t + ct[:, 3:4] * p[1:-1, 2:]
    t = t + ct[:, 4:5] * p[2:, 1:-1]
    return t


def half_sweep(ct, dinv, scale, b, u, c):
    res = b - apply(ct, u)
    new = u + scale * (res * np.asarray(dinv).reshape(-1, 1))
    return np.where(colour(*u.shape) == c, new, u)


def sweeps(ct, dinv, scale, b, u, nsweeps):
    """nsweeps red-black sweeps; u None: from the zero guess"""
    u = np.zeros_like(b) if u is None else u
    for _ in range(nsweeps):
        u = half_sweep(ct, dinv, scale, b, u, 0)
        u = half_sweep(ct, dinv, scale, b, u, 1)
    return u


def const_table(coef, dinv, ny):
    """the row tables of a constant five-point stencil {S, W, C, E, N}"""
    return np.tile(np.asarray(coef, dtype=np.float64), (ny, 1)), np.full(ny, float(dinv))


class Hierarchy:
    """the level tables of one configuration"""

    def __init__(self, orc, npts, levels, mesh):
        self.orc, self.npts, self.levels, self.mesh = orc, npts, levels, mesh
        self.n = [orc.L.mgo_grid_n(npts, l) for l in range(levels)]
        self.ct = [LR.level_table(orc, npts, l, mesh) for l in range(levels)]
        self.dinv = [1.0 / ct[:, 2] for ct in self.ct]

    def rhs(self):
        return self.orc.rhs_mesh(self.npts, self.mesh) if self.mesh else self.orc.rhs(2, self.npts)

    def smooth(self, l, scale, b, u, its):
        """KSPSolve with max_it = its; u None: from the zero guess"""
        if its == 0 and u is None:
            return np.zeros_like(b)
        if its == 0:
            return u
        return sweeps(self.ct[l], self.dinv[l], scale, b, u, its)

    def residual(self, l, b, u):
        return b - apply(self.ct[l], u)


def solve(h, b, scale, v=(3, 3), rtol=1.0e-7, maxiter=100):
    """the loop of the reference driver (src/solver.c:1512-1550) with red-black sweeps; returns {"iters", "rnorm", "u", "bnorm"}"""
    orc, L, n = h.orc, h.levels, h.n
    b0 = np.ascontiguousarray(b, dtype=np.float64).reshape(n[0], n[0])
    norm = lambda x: math.sqrt(orc.sumsq(np.ascontiguousarray(x).ravel()))
    bnorm = norm(b0)
    u = [None] * L
    bb = [b0] + [None] * (L - 1)
    rchk = norm(b0)                                             # b - A 0
    rn, it = [rchk], 0
    while it < maxiter and 100000000 * bnorm > rchk and rchk > rtol * bnorm:
        u[0] = h.smooth(0, scale, bb[0], u[0], v[0])
        for l in range(1, L):
            r = h.residual(l - 1, bb[l - 1], u[l - 1])
            bb[l] = orc.restrict(2, n[l - 1], np.ascontiguousarray(r).ravel()).reshape(n[l], n[l])
            u[l] = h.smooth(l, scale, bb[l], None, v[1] if l == L - 1 else v[0])
        for l in range(L - 2, -1, -1):
            u[l] = orc.prolong_add(2, n[l], np.ascontiguousarray(u[l + 1]).ravel(), np.ascontiguousarray(u[l]).ravel()).reshape(n[l], n[l])
            u[l] = h.smooth(l, scale, bb[l], u[l], v[0])
        rchk = norm(h.residual(0, bb[0], u[0]))
        it += 1
        rn.append(rchk)
    u0 = np.zeros_like(b0) if u[0] is None else u[0]
    return {"iters": it, "rnorm": np.array(rn), "u": np.ascontiguousarray(u0).ravel(), "bnorm": bnorm}


RTOL = 1.0e-7
LEVELS = {17: 4, 33: 5, 65: 6, 129: 7, 513: 9}                 # levels down to 1 x 1
_REF, _HIER = {}, {}


def hierarchy(orc, npts, mesh):
    if (npts, mesh) not in _HIER:
        _HIER[(npts, mesh)] = Hierarchy(orc, npts, LEVELS[npts], mesh)
    return _HIER[(npts, mesh)]


def case_key(case):
    return ",".join(repr(c) if isinstance(c, float) else str(c) for c in case)


def case_rhs(h, rhs):
    """'manufactured', 'rough:<seed>' (rhs_cases.uniform) or 'spikes:<seed>'"""
    import rhs_cases
    if rhs == "manufactured":
        return h.rhs()
    fam, seed = rhs.split(":")
    return rhs_cases.make("uniform" if fam == "rough" else fam, 2, h.npts, int(seed))


def reference(orc, case):
    """the reference solve of a case (npts, mesh, scale, v0, v1, rhs), levels down to 1 x 1: computed once per process and never changed"""
    if case not in _REF:
        npts, mesh, scale, v0, v1, rhs = case
        h = hierarchy(orc, npts, mesh)
        _REF[case] = solve(h, case_rhs(h, rhs), scale, v=(v0, v1), rtol=RTOL, maxiter=100)
    return _REF[case]


def compare(ref, it, rn, u, bnorm):
    """a solve of the product against the reference: the same count, the history within 1e-12 (relative, entry by entry), u bit for bit.  The
    count is compared under the margin rule of tests/test_gmres_solve_gpu.py (gmres_reference.margins: the last norm <= 0.8, the one before >= 1.5
    in units of rtol ||b||); a reference that stops closer to the threshold than that must at least stay clear of it by 1e-6
    (rhs_cases.stop_rule_clear), a million times the 1e-12 between two orders of summation, and one that ran into maxiter has no stop decision"""
    import gmres_reference as G
    import rhs_cases
    last, before = G.margins(ref, RTOL)
    if not (last <= 0.8 and before >= 1.5) and ref["iters"] < 100:
        assert rhs_cases.stop_rule_clear(ref, RTOL), (last, before)
    assert it == ref["iters"], (it, ref["iters"])
    rn = np.asarray(rn)
    assert len(rn) == it + 1 and abs(bnorm - ref["bnorm"]) <= 1e-13 * ref["bnorm"]
    rel = np.abs(rn - ref["rnorm"]) / ref["rnorm"]
    assert rel.max() <= 1e-12, rel.max()
    assert np.array_equal(np.asarray(u), ref["u"])
