"""y-line Jacobi in numpy: the definition that mgk_line_forward_f64 / mgk_line_backward_f64 (csrc/mgk_line.hip), the host tables of
csrc/mg_line.c and the cycle of Solver(pc_type="yline") are held to, operation for operation.  Test infrastructure only.

Level with n x n unknowns, row i with the coefficients {S, W, C, E, N}_i = ct[i, 0..4] (tests/row_tables.py).  T = the y-tridiagonal part of A:

  tables   m_0 = C_0, g_0 = 1/m_0, l_0 = 0;  i >= 1: l_i = S_i g_{i-1}, m_i = C_i - l_i N_{i-1}, g_i = 1/m_i;  q_i = N_i g_i
  sweep    r_i = b_i - (A u)_i          the five terms in the order of _rt_apply; from the zero guess r = b and u is not read
           y_0 = r_0, y_i = r_i - l_i y_{i-1};  z_i = y_i g_i
           e_{n-1} = z_{n-1}, e_i = z_i - q_i e_{i+1};  u'_i = u_i + s e_i; from the zero guess u'_i = s e_i

Every product and every sum is rounded on its own (numpy does not contract).  Python loops over rows, vectorised over columns.  The cycle is
the loop of oracle/mgo.c's mgo_vcycle with these sweeps as the smoother, _rt_apply for A u, Oracle.restrict / Oracle.prolong_add for the
transfers and Oracle.sumsq for the norms; the row tables of a level come from the oracle's ASSEMBLED rows (mgo_build_A / mgo_build_A_mesh),
not from the product."""
import ctypes as C
import math

import numpy as np

from row_tables import _rt_apply


def tables(ct):
    """(l, g, q) of the y-tridiagonal part of the row-table operator ct (n x 5)"""
    n = ct.shape[0]
    l, g, q = np.zeros(n), np.zeros(n), np.zeros(n)
    m = ct[0, 2]
    g[0] = 1.0 / m
    for i in range(1, n):
        l[i] = ct[i, 0] * g[i - 1]
        t = l[i] * ct[i - 1, 4]
        m = ct[i, 2] - t
        g[i] = 1.0 / m
    for i in range(n):
        q[i] = ct[i, 4] * g[i]
    return l, g, q


def forward(ct, l, g, b, u=None):
    """z (n x n) of one sweep; u None: the zero guess"""
    n = b.shape[0]
    r = b if u is None else b - _rt_apply(ct, u)
    z = np.empty_like(b)
    y = r[0].copy()
    z[0] = y * g[0]
    for i in range(1, n):
        t = l[i] * y
        y = r[i] - t
        z[i] = y * g[i]
    return z


def backward(q, scale, z, u=None):
    n = z.shape[0]
    out = np.empty_like(z)
    e = z[n - 1].copy()
    se = scale * e
    out[n - 1] = se if u is None else u[n - 1] + se
    for i in range(n - 2, -1, -1):
        t = q[i] * e
        e = z[i] - t
        se = scale * e
        out[i] = se if u is None else u[i] + se
    return out


def sweep(ct, tab, scale, b, u=None):
    l, g, q = tab
    return backward(q, scale, forward(ct, l, g, b, u), u)


def level_table(orc, npts, l, mesh):
    """ct (n x 5) of level l from the oracle's assembled operator: the entries of the rows of ONE interior column (the rows depend on the
    grid row only), by column offset -n, -1, 0, +1, +n; an entry the boundary drops (it would multiply a zero) is 0"""
    m = orc.L.mgo_build_A_mesh(npts, l, mesh) if mesh else orc.L.mgo_build_A(2, npts, l)
    n = orc.L.mgo_grid_n(npts, l)
    assert orc.L.mgo_csr_nrows(m) == n * n
    j = min(1, n - 1)
    ct = np.zeros((n, 5))
    cols, vals, cnt = np.zeros(64, dtype=np.int32), np.zeros(64), C.c_int()
    slot = {-n: 0, -1: 1, 0: 2, 1: 3, n: 4}
    for i in range(n):
        row = i * n + j
        orc.L.mgo_csr_row(m, row, C.byref(cnt), cols.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p))
        for c, v in zip(cols[:cnt.value], vals[:cnt.value]):
            ct[i, slot[int(c) - row]] = v
    orc.L.mgo_csr_free(m)
    return ct


class Hierarchy:
    """the level tables of one configuration"""

    def __init__(self, orc, npts, levels, mesh):
        self.orc, self.npts, self.levels, self.mesh = orc, npts, levels, mesh
        self.n = [orc.L.mgo_grid_n(npts, l) for l in range(levels)]
        self.ct = [level_table(orc, npts, l, mesh) for l in range(levels)]
        self.tab = [tables(ct) for ct in self.ct]

    def rhs(self):
        b = self.orc.rhs_mesh(self.npts, self.mesh) if self.mesh else self.orc.rhs(2, self.npts)
        return b

    def smooth(self, l, scale, b, u, its):
        """KSPSolve with max_it = its; u None: from the zero guess"""
        if its == 0 and u is None:
            return np.zeros_like(b)
        for _ in range(its):
            u = sweep(self.ct[l], self.tab[l], scale, b, u)
        return u

    def residual(self, l, b, u):
        return b - _rt_apply(self.ct[l], u)


def solve(h, b, scale, v=(3, 3), rtol=1.0e-7, maxiter=100):
    """the loop of the reference driver (src/solver.c:1512-1550) with y-line sweeps; returns {"iters", "rnorm", "u", "bnorm"}"""
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


def margins(ref, rtol=1.0e-7):
    """(last norm, the one before) in units of rtol ||b||: the stop decision is clear of rounding when the first is <= 0.8 and the
    second >= 1.5"""
    qq = ref["rnorm"] / (rtol * ref["bnorm"])
    return float(qq[-1]), float(qq[-2])


SCALE = 0.8
RTOL = 1.0e-7
# (npts, levels, mesh, rhs): levels down to 1 x 1; rhs "manufactured" or "rough:<seed>" (tests/rhs_cases.uniform).  The seeds are the first
# whose stop decision on THIS reference is clear of rounding (margins <= 0.8 and >= 1.5; a seed that is not gets replaced, never skipped)
CASES = [(npts, levels, mesh, rhs) for npts, levels, mesh, seed in ((65, 6, 0, 3), (65, 6, 1, 3), (129, 7, 0, 3), (129, 7, 1, 3), (17, 4, 2, 6))
         for rhs in ("manufactured", f"rough:{seed}")]
_REF = {}


def case_key(case):
    return ",".join(str(c) for c in case)


def case_rhs(h, rhs):
    import rhs_cases
    return h.rhs() if rhs == "manufactured" else rhs_cases.uniform(2, h.npts, int(rhs.split(":")[1]))


def reference(orc, case):
    """the reference solve of a case, computed once per process and never changed"""
    if case not in _REF:
        npts, levels, mesh, rhs = case
        h = Hierarchy(orc, npts, levels, mesh)
        _REF[case] = solve(h, case_rhs(h, rhs), SCALE, rtol=RTOL, maxiter=100)
    return _REF[case]


def compare(ref, it, rn, u, bnorm):
    """a solve of the product against the reference: the same count (compared only where the reference's stop decision is clear of rounding),
    the history within 1e-12 of rnorm[0], u bit for bit"""
    last, before = margins(ref, RTOL)
    assert last <= 0.8 and before >= 1.5, (last, before)
    assert it == ref["iters"], (it, ref["iters"])
    rn = np.asarray(rn)
    assert len(rn) == it + 1 and abs(bnorm - ref["bnorm"]) <= 1e-13 * ref["bnorm"]
    assert np.abs(rn - ref["rnorm"]).max() <= 1e-12 * ref["rnorm"][0], np.abs(rn - ref["rnorm"]).max() / ref["rnorm"][0]
    assert np.array_equal(np.asarray(u), ref["u"])
