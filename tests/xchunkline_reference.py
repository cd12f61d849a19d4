"""Chunked x-line Jacobi in numpy: the definition that the four mgk_xline_chunk_*_f64 passes (csrc/mgk_xline_chunk.hip),
the host tables of csrc/mg_xline_chunk.c and the cycle of Solver(pc_type="xline" / "altline", xline_chunk=c) are held to, operation for
operation.  Test infrastructure only.  Section 8h (tests/chunkline_reference.py) turned by 90 degrees: a partitioned (separator / Schur
complement) solve of the x-tridiagonal systems T_x x = r of tests/xline_reference.py.  A level has nx columns and ny rows; grid row i has
{S, W, C, E, N}_i = ct[i, 0..4] and T_x is in that row the constant-band matrix (W_i, C_i, E_i).  Period c, a multiple of 16, K = nx // c:

  layout   separator column q (0 <= q < K): s_q = q c + c - 1;  chunk k (0 <= k <= K): the columns [a_k, b_k), a_k = k c,
           b_k = min(k c + c - 1, nx) (the last chunk is empty when nx = K c; K = 0: the sweep is xline_reference.sweep to the bit)
  tables   g: xline_reference.table restarted in every chunk (g_a = 1 / C; j > a: l = W g_{j-1}, t = l E, m = C - t, g_j = 1 / m), a stored 0
           in the separator columns; the multipliers l_j = W g_{j-1} and q_j = E g_j are one rounded product each, formed in the sweep
           spikes v = T_k^-1 (W e_a), w = T_k^-1 (E e_{b-1}) by the two substitutions of the sweep on that right-hand side; v = 0 on chunk 0,
           w = 0 on chunk K, both 0 in the separator columns (STORED zeros)
           Schur rows d = (C - W w[s-1]) - E v[s+1], sub = -(W v[s-1]), sup = -(E w[s+1]); s = nx - 1: d = C - W w[s-1], sup = 0
           SL, SG, SQ: the recurrence of chunkline_reference._factor on (sub, d, sup) along q, per row
  sweep    r as xline_reference; in every chunk y_a = r_a, y_j = r_j - l_j y_{j-1}, z_j = y_j g_j; x'_{b-1} = z_{b-1}, x'_j = z_j - q_j x'_{j+1}
           rho_q = (r_s - W x'_{s-1}) - E x'_{s+1} (the last term omitted when s = nx - 1); Y_0 = rho_0, Y_q = rho_q - SL_q Y_{q-1},
           Z_q = Y_q SG_q; xi_{K-1} = Z_{K-1}, xi_q = Z_q - SQ_q xi_{q+1}
           x_j = (x'_j - xi_{k-1} v_j) - xi_k w_j in chunk k (the first term OMITTED for k = 0, the second for k = K); x_s = xi_q
           u' = u + scale x; from the zero guess u' = scale x

Every product and every sum is rounded on its own.  Python loops over columns, vectorised over rows.  The four functions forward / backward /
reduce / correct return what the four passes leave in memory: the scratch field t (z on the chunk columns with the unmodified r_s in the
separator columns, then x' on the chunk columns) and the separator workspace, four planes R, XL, XR, XI of K rows of ny values each
(R[q] = r_s, XL[q] = x'_{s-1}, XR[q] = x'_{s+1}, XI[q] = xi_q).  An entry the definition never forms -- XR[K-1] when s_{K-1} = nx - 1 -- is NaN
here and stays unwritten and unread in the product."""
import numpy as np

import chunkline_reference as CR
import line_reference as LR
import xline_reference as XR


def layout(nx, c):
    """(K, chunks [(a, b)] for k = 0 .. K, separator columns)"""
    assert c > 0 and c % 16 == 0
    K = nx // c
    return K, [(k * c, min(k * c + c - 1, nx)) for k in range(K + 1)], [q * c + c - 1 for q in range(K)]


def _chunk_solve(ct, g, a, b, x):
    """the two substitutions of the sweep on the columns [a, b) of x (rows x columns), in place: r -> x'"""
    y = x[:, a].copy()
    x[:, a] = y * g[:, a]
    for j in range(a + 1, b):
        l = ct[:, 1] * g[:, j - 1]
        t = l * y
        y = x[:, j] - t
        x[:, j] = y * g[:, j]
    e = x[:, b - 1].copy()
    for j in range(b - 2, a - 1, -1):
        q = ct[:, 3] * g[:, j]
        t = q * e
        e = x[:, j] - t
        x[:, j] = e


def tables(ct, c, nx=None):
    """the tables of period c on nx columns (the number of rows unless given): a dict with c, K, g, v, w (ny x nx) and sub, d, sup, SL, SG,
    SQ (ny x K)"""
    ny = ct.shape[0]
    nx = ny if nx is None else nx
    K, chunks, seps = layout(nx, c)
    W, Cc, E = ct[:, 1], ct[:, 2], ct[:, 3]
    g, v, w = (np.zeros((ny, nx)) for _ in range(3))
    for k, (a, b) in enumerate(chunks):
        if b <= a:
            continue
        g[:, a:b] = XR.table(ct, b - a)
        if k > 0:
            x = np.zeros((ny, nx))
            x[:, a] = W
            _chunk_solve(ct, g, a, b, x)
            v[:, a:b] = x[:, a:b]
        if k < K:
            x = np.zeros((ny, nx))
            x[:, b - 1] = E
            _chunk_solve(ct, g, a, b, x)
            w[:, a:b] = x[:, a:b]
    sub, d, sup = (np.zeros((ny, K)) for _ in range(3))
    for q, s in enumerate(seps):
        t = W * w[:, s - 1]
        d[:, q] = Cc - t
        t = W * v[:, s - 1]
        sub[:, q] = -t
        if s < nx - 1:
            t = E * v[:, s + 1]
            d[:, q] = d[:, q] - t
            t = E * w[:, s + 1]
            sup[:, q] = -t
    SL, SG, SQ = (np.zeros((ny, K)) for _ in range(3))
    for i in range(ny):
        SL[i], SG[i], SQ[i] = CR._factor(sub[i], d[i], sup[i])
    return dict(c=c, K=K, g=g, v=v, w=w, sub=sub, d=d, sup=sup, SL=SL, SG=SG, SQ=SQ)


def _sep(K, ny):
    return {p: np.full((K, ny), np.nan) for p in ("R", "XL", "XR", "XI")}


def forward(ct, tab, b, u=None):
    """(t, sep): z on the chunk columns, the unmodified residual r_s in the separator columns and in R; u None: the zero guess"""
    ny, nx = b.shape
    K, chunks, seps = layout(nx, tab["c"])
    g = tab["g"]
    r = b if u is None else b - CR._apply(ct, u)
    t = np.empty_like(b)
    for a, e in chunks:
        if e <= a:
            continue
        y = r[:, a].copy()
        t[:, a] = y * g[:, a]
        for j in range(a + 1, e):
            l = ct[:, 1] * g[:, j - 1]
            p = l * y
            y = r[:, j] - p
            t[:, j] = y * g[:, j]
    sep = _sep(K, ny)
    for q, s in enumerate(seps):
        t[:, s] = r[:, s]
        sep["R"][q] = r[:, s]
    return t, sep


def backward(ct, tab, t, sep):
    """(t, sep): x' on the chunk columns, the separator columns kept; XL[q] = x' left of separator q, XR[q] = x' right of it (if there is one)"""
    ny, nx = t.shape
    K, chunks, seps = layout(nx, tab["c"])
    g = tab["g"]
    x = t.copy()
    sep = {p: a.copy() for p, a in sep.items()}
    for k, (a, e) in enumerate(chunks):
        if e <= a:
            continue
        ee = x[:, e - 1].copy()
        for j in range(e - 2, a - 1, -1):
            q = ct[:, 3] * g[:, j]
            p = q * ee
            ee = x[:, j] - p
            x[:, j] = ee
        if k < K:
            sep["XL"][k] = x[:, e - 1]
        if k > 0:
            sep["XR"][k - 1] = x[:, a]
    return x, sep


def reduce(ct, tab, sep, nx):
    """sep with XI[q] = xi_q; R, XL and XR unchanged"""
    K, _, seps = layout(nx, tab["c"])
    SL, SG, SQ = tab["SL"], tab["SG"], tab["SQ"]
    sep = {p: a.copy() for p, a in sep.items()}
    Y = None
    for q, s in enumerate(seps):
        p = ct[:, 1] * sep["XL"][q]
        rho = sep["R"][q] - p
        if s < nx - 1:
            p = ct[:, 3] * sep["XR"][q]
            rho = rho - p
        if q == 0:
            Y = rho
        else:
            p = SL[:, q] * Y
            Y = rho - p
        sep["XI"][q] = Y * SG[:, q]
    for q in range(K - 2, -1, -1):
        p = SQ[:, q] * sep["XI"][q + 1]
        sep["XI"][q] = sep["XI"][q] - p
    return sep


def correct(tab, scale, t, sep, u=None):
    """u' from x' and xi"""
    ny, nx = t.shape
    K, chunks, seps = layout(nx, tab["c"])
    v, w = tab["v"], tab["w"]
    x = t.copy()
    for k, (a, e) in enumerate(chunks):
        for j in range(a, e):
            xj = t[:, j]
            if k > 0:
                p = sep["XI"][k - 1] * v[:, j]
                xj = xj - p
            if k < K:
                p = sep["XI"][k] * w[:, j]
                xj = xj - p
            x[:, j] = xj
    for q, s in enumerate(seps):
        x[:, s] = sep["XI"][q]
    se = scale * x
    return se if u is None else u + se


def sweep(ct, tab, scale, b, u=None):
    t, sep = forward(ct, tab, b, u)
    t, sep = backward(ct, tab, t, sep)
    sep = reduce(ct, tab, sep, b.shape[1])
    return correct(tab, scale, t, sep, u)


class Hierarchy(CR.Hierarchy):
    """pc "xline": x sweeps; "altline": sweep k of a smoothing is a y sweep for even k and an x sweep for odd k.  The y sweeps of the levels
    with n >= yc > 0 are those of tests/chunkline_reference.py, the x sweeps of the levels with n >= xc > 0 the chunked ones of this file;
    every other sweep is the plain one"""

    def __init__(self, orc, npts, levels, mesh, pc, xc, yc=0):
        super().__init__(orc, npts, levels, mesh, yc)
        assert pc in ("xline", "altline")
        self.pc, self.xc = pc, xc
        self.xg = [XR.table(ct) for ct in self.ct]
        self.xtab = [tables(ct, xc) if xc > 0 and ct.shape[0] >= xc else None for ct in self.ct]

    def xsweep(self, l, scale, b, u):
        if self.xtab[l] is None:
            return XR.sweep(self.ct[l], self.xg[l], scale, b, u)
        return sweep(self.ct[l], self.xtab[l], scale, b, u)

    def smooth(self, l, scale, b, u, its):
        if its == 0 and u is None:
            return np.zeros_like(b)
        for k in range(its):
            u = self.ysweep(l, scale, b, u) if (self.pc == "altline" and k % 2 == 0) else self.xsweep(l, scale, b, u)
        return u


_REF = {}


def reference(orc, case, pc, xc, yc=0):
    """the reference solve of a case (npts, levels, mesh, rhs), computed once per process and never changed"""
    key = (case, pc, xc, yc)
    if key not in _REF:
        npts, levels, mesh, rhs = case
        h = Hierarchy(orc, npts, levels, mesh, pc, xc, yc)
        _REF[key] = LR.solve(h, LR.case_rhs(h, rhs), LR.SCALE, rtol=LR.RTOL, maxiter=100)
    return _REF[key]
