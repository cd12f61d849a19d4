"""Restarted, right-preconditioned GMRES in numpy over the CPU oracle: the definition that mg_solver_solve_gmres (csrc/mg_gmres.c) is held to.
Test infrastructure only.

  M r   one V(3,3) cycle from the zero guess: Oracle.vcycle(fixed_cycles=1, b=r), the assembled leg (use_csr=1) on the stretched meshes
  A x   Oracle.apply with the level-0 stencil; csr_mult on mgo_build_A_mesh on the stretched meshes

  x = 0, r = b, beta = ||b||, v_0 = r / beta
  step j: w = A (M v_j); h_i = v_i . w for i <= j (classical Gram-Schmidt, one pass, no refinement); w <- (..(w - h_0 v_0)..) - h_j v_j;
          h_{j+1} = ||w||; Givens rotations; estimate |g_{j+1}|; v_{j+1} = w * (1 / h_{j+1})
  stop when the estimate is <= rtol ||b||, at maxiter steps, under the divergence guard (1e8 ||b|| <= estimate), or after `restart` steps:
          H y = g, x <- x + M (V y); going on from r = b - A x, beta = ||r||

The sums (dots, norms) have no fixed order on the GPU, so two variants are selectable: dot="np" (np.dot: blocked, pairwise) and dot="ld" (a
long-double sum).  The distance between the two is the measure of what rounding alone does to a solve (tests/test_gmres_solve_gpu.py)."""
import math

import numpy as np


def _dot(kind):
    if kind == "np":
        return lambda a, b: float(np.dot(a, b))
    if kind == "ld":
        return lambda a, b: float(np.sum(a.astype(np.longdouble) * b.astype(np.longdouble), dtype=np.longdouble))
    raise ValueError(kind)


class Operators:
    """A and M of one configuration, on compact lexicographic fields"""

    def __init__(self, orc, dim, npts, levels, mesh, scale, v=(3, 3)):
        self.orc, self.dim, self.npts, self.levels, self.mesh, self.scale, self.v = orc, dim, npts, levels, mesh, scale, v
        self.n = npts - 2
        self.napply = 0
        if mesh:
            self.csr = orc.L.mgo_build_A_mesh(npts, 0, mesh)
        else:
            self.csr = None
            self.As = orc.level_stencil(dim, npts, 0)[0]

    def close(self):
        if self.csr:
            self.orc.L.mgo_csr_free(self.csr)
            self.csr = None

    def A(self, x):
        if self.csr:
            return self.orc.csr_mult(self.csr, x)
        return self.orc.apply(self.dim, self.n, self.As, x)

    def M(self, r):
        self.napply += 1
        return self.orc.vcycle(self.dim, self.npts, self.levels, self.v[0], self.v[1], maxiter=1, scale=self.scale,
                               use_csr=1 if self.mesh else 0, fixed_cycles=1, mesh=self.mesh, b=r)["u"]

    def rhs(self):
        """the manufactured right-hand side of the configuration"""
        return self.orc.rhs_mesh(self.npts, self.mesh) if self.mesh else self.orc.rhs(self.dim, self.npts)


def gmres(op, b, restart, rtol=1.0e-7, maxiter=100000, dot="np"):
    """returns {"iters", "rnorm" (rnorm[0] = ||b||, rnorm[k] = the estimate after step k), "x", "bnorm", "napply" (applications of M),
    "true" (||b - A x||)}"""
    dt = _dot(dot)
    b = np.ascontiguousarray(b, dtype=np.float64)
    bnorm = math.sqrt(dt(b, b))
    tol = rtol * bnorm
    x = np.zeros_like(b)
    rn = [bnorm]
    it, napply0 = 0, op.napply
    if bnorm == 0.0 or maxiter < 1:
        return {"iters": 0, "rnorm": np.array(rn), "x": x, "bnorm": bnorm, "napply": 0, "true": bnorm}
    r, beta, res, first = b, bnorm, bnorm, True

    def go_on():
        return it < maxiter and 100000000 * bnorm > res and res > tol

    while go_on():
        V = [(1.0 / beta) * r]
        g = [beta]
        H, cs, sn = [], [], []
        j = 0
        while True:
            w = op.A(op.M(V[j]))
            h = [dt(V[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = w - h[i] * V[i]
            hn = math.sqrt(dt(w, w))
            for i in range(j):
                t = cs[i] * h[i] + sn[i] * h[i + 1]
                h[i + 1] = cs[i] * h[i + 1] - sn[i] * h[i]
                h[i] = t
            d = math.sqrt(h[j] * h[j] + hn * hn)
            c, s = (1.0, 0.0) if d == 0.0 else (h[j] / d, hn / d)
            cs.append(c); sn.append(s)
            h[j] = c * h[j] + s * hn
            g.append(-(s * g[j]))
            g[j] = c * g[j]
            H.append(h)
            res = abs(g[j + 1])
            it += 1
            rn.append(res)
            j += 1
            if not (j < restart and go_on()):
                break
            V.append((1.0 / hn) * w)
        y = [0.0] * j
        for i in range(j - 1, -1, -1):
            t = g[i]
            for q in range(i + 1, j):
                t -= H[q][i] * y[q]
            y[i] = t / H[i][i] if H[i][i] != 0.0 else 0.0
        t = y[0] * V[0]
        for i in range(1, j):
            t = t + y[i] * V[i]
        mt = op.M(t)
        x = mt if first else x + mt
        first = False
        if not go_on():
            break
        r = b - op.A(x)
        beta = math.sqrt(dt(r, r))
        res = beta
    rt = b - op.A(x)
    return {"iters": it, "rnorm": np.array(rn), "x": x, "bnorm": bnorm, "napply": op.napply - napply0, "true": math.sqrt(float(np.dot(rt, rt)))}


def margins(ref, rtol=1.0e-7):
    """(last estimate, the one before) in units of rtol ||b||: the stop decision is clear of rounding when the first is <= 0.8 and the
    second >= 1.5"""
    q = ref["rnorm"] / (rtol * ref["bnorm"])
    return float(q[-1]), float(q[-2])


def delta(a, b):
    """the larger of max|x_a - x_b| / max|x_b| and max_k |rnorm_a[k] - rnorm_b[k]| / rnorm[0] (histories of equal length)"""
    dx = float(np.abs(a["x"] - b["x"]).max() / np.abs(b["x"]).max())
    n = min(len(a["rnorm"]), len(b["rnorm"]))
    dr = float(np.abs(a["rnorm"][:n] - b["rnorm"][:n]).max() / b["rnorm"][0])
    return max(dx, dr)


def distance(x, rnorm, ref):
    """the same two quantities between a result (x, rnorm) and one variant of the reference"""
    return delta({"x": np.asarray(x), "rnorm": np.asarray(rnorm)}, ref)


def judge(orc, config, b, refs, it, rn, x, bnorm, rtol=1.0e-7):
    """The bars a solve_gmres result (it, rn, x, bnorm) is held to, on config = (dim, npts, levels, mesh, scale) and the right-hand side b,
    against refs = the reference's two orders of summation (dot="np", "ld"): a stop decision clear of rounding in both, the same count, the
    history's length and its first entry, x and the history within 100 delta of the nearer variant (delta = the distance between the two,
    floor 1e-13), and a converged TRUE residual.  Shared by tests/test_gmres_cpu.py and the session draw (tools/stress_sessions_mock.py)."""
    dim, npts, levels, mesh, scale = config
    for r in refs:
        last, before = margins(r, rtol)
        assert last <= 0.8 and before >= 1.5, (last, before)
    assert it == refs[0]["iters"] == refs[1]["iters"]
    assert len(rn) == it + 1 and rn[0] == bnorm and abs(bnorm - refs[0]["bnorm"]) <= 1e-13 * bnorm
    bound = max(100.0 * delta(refs[0], refs[1]), 1e-13)
    dist = min(distance(x, rn, r) for r in refs)
    assert dist <= bound, (dist, bound)
    op = Operators(orc, dim, npts, levels, mesh, scale)
    r = b - op.A(x)
    op.close()
    eps = max(abs(q["rnorm"][-1] - q["true"]) / q["true"] for q in refs)
    assert np.sqrt(np.dot(r, r)) <= rtol * bnorm * (1.0 + 100.0 * eps)
