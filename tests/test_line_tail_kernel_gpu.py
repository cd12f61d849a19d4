"""mgk_tail_cycle_line_f64 (csrc/mgk_line_tail.hip), called directly, against numpy: the LDS-resident coarse levels of a line cycle in one launch.

  reference      the tail on the levels t .. L-1 with input b is exactly ONE cycle from the zero guess of the sub-hierarchy rooted at t:
                 XR.Hierarchy viewed from level t (n, ct, tab, xg sliced), XR.solve(view, b, scale, v, rtol=0, maxiter=1)["u"].  (A view of ONE
                 level is the coarsest level alone: it takes v1 sweeps, which the reference's loop spells v[0].)
  bar            np.array_equal on u, and np.signbit wherever the value is 0
  cases          pc y / x / alt x mesh 0 / 1 / 2 x (npts, levels, t) giving n[0] = 1, 3, 7, 15, 31, 63 and 15 with 1 .. 6 levels; in each,
                 v = (3, 3), (2, 1), (1, 2), (0, 1) and scale 0.8 and 1.0; b uniform(-1, 1), seeded
  device tables  as the product makes them: on mesh 0 the level's five constants in every row and ONE row of the x table (stride 0); on
                 meshes 1 / 2 the oracle's assembled rows and an n x n x table at a stride of n rounded up to 16 doubles, the padding a sentinel
  row tables     one set on non-symmetric row tables (S != N, W != E, varying with the row: tests/coef_cases.distinct_row_tables) -- the
                 Poisson tables cannot tell a swapped neighbour; the reference sweeps run on the same tables
  surroundings   u starts from a sentinel everywhere (ghost ring, padding, 256 doubles past the field) and keeps it outside the interior;
                 b is unchanged
  refusals       3-D, levels that do not fit, a hierarchy that is none, a null table the chosen pc needs, bad counts: MGK_EINVAL, each with
                 its message"""
import copy
import ctypes as C

import numpy as np
import pytest

import line_reference as LR
import xline_reference as XR
from coef_cases import distinct_row_tables
from oracle import Oracle

pytestmark = pytest.mark.gpu
SENT = 12345.678
PCS = {"yline": 1, "xline": 2, "altline": 3}
SHAPES = [(5, 2, 1), (9, 3, 1), (17, 4, 1), (33, 5, 1), (65, 6, 1), (129, 7, 1), (129, 7, 3)]     # n[0] = 1, 3, 7, 15, 31, 63, 15
VS = [(3, 3), (2, 1), (1, 2), (0, 1)]
SCALES = [0.8, 1.0]
MGK_EINVAL = 10001
_H = {}


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _hierarchy(orc, npts, levels, mesh, pc):
    """the level tables of a configuration, built once per process (the smoothing depends on pc alone: a shallow copy serves each)"""
    key = (npts, levels, mesh)
    if key not in _H:
        _H[key] = XR.Hierarchy(orc, npts, levels, mesh, "altline")
    h = copy.copy(_H[key])
    h.pc, h.log = pc, []
    return h


def _view(h, t):
    v = copy.copy(h)
    v.n, v.ct, v.tab, v.xg, v.levels, v.log = h.n[t:], h.ct[t:], h.tab[t:], h.xg[t:], h.levels - t, []
    return v


def _reference(view, b, scale, v):
    vv = (v[1], v[1]) if view.levels == 1 else v          # the coarsest level alone: v1 sweeps
    return XR.solve(view, b, scale, v=vv, rtol=0.0, maxiter=1)["u"].reshape(view.n[0], view.n[0])


def _index(g):
    return g.org + np.arange(g.ny)[:, None] * g.pitch + np.arange(g.nx)[None, :]


def _put(mgk, g, inner, fill=SENT):
    raw = np.full(g.total + 256, fill)
    if inner is not None:
        raw[_index(g)] = inner
    return mgk.upload(raw)


def _get(mgk, g, p, fill=SENT):
    """the interior; everything else must still hold `fill`"""
    raw = mgk.download(p, g.total + 256)
    idx = _index(g)
    inner = raw[idx].copy()
    raw[idx] = fill
    assert np.all(raw == fill), "a cell outside the interior was written"
    return inner


class _Tables:
    """the device tables of the levels of a view, as the product uploads them"""

    def __init__(self, mgk, cts, uniform):
        self.mgk, self.ptrs = mgk, []
        self.ct, self.lt, self.gt, self.qt, self.xg, self.xgs = [], [], [], [], [], []
        for ct in cts:
            n = ct.shape[0]
            if uniform:
                ct = np.tile(ct[min(1, n - 1)], (n, 1))      # the level's five constants in every row
            l, g, q = LR.tables(ct)
            x = XR.table(ct)
            if uniform:
                xdev, gs = np.concatenate([x[0], np.full(3, SENT)]), 0
            else:
                gs = (n + 15) // 16 * 16
                xdev = np.full((n, gs), SENT)
                xdev[:, :n] = x
                xdev = xdev.ravel()
            for arr, dst in ((ct, self.ct), (l, self.lt), (g, self.gt), (q, self.qt), (xdev, self.xg)):
                p = mgk.upload(arr)
                self.ptrs.append(p)
                dst.append(p)
            self.xgs.append(gs)

    def args(self, pc):
        y, x = pc != 2, pc != 1
        return dict(ctab=self.ct, ltab=self.lt if y else None, gtab=self.gt if y else None, qtab=self.qt if y else None,
                    xgtab=self.xg if x else None, xgs=self.xgs if x else None)

    def free(self):
        for p in self.ptrs:
            self.mgk.free(p)


def _check(mgk, view, tabs, pc, seed):
    """every v and scale on one view: u against the reference, bit for bit and sign for sign; u's surroundings and b untouched"""
    n = view.n
    g = mgk.geom(2, n[0])
    rng = np.random.default_rng(seed)
    for v in VS:
        for scale in SCALES:
            b = rng.uniform(-1, 1, (n[0], n[0]))
            ref = _reference(view, b, scale, v)
            db, du = _put(mgk, g, b), _put(mgk, g, None)
            mgk._chk(mgk.tail_cycle_line(g, n, PCS[pc], scale=scale, v=v, b=db, u=du, **tabs.args(PCS[pc])))
            mgk.sync()
            u = _get(mgk, g, du)
            assert np.array_equal(_get(mgk, g, db), b), "b was written"
            mgk.free(db)
            mgk.free(du)
            bad = int(np.sum(u != ref))
            print(f"{pc} n = {n} v = {v} scale = {scale}: u differs in {bad} of {u.size}")
            assert np.array_equal(u, ref), (pc, n, v, scale, bad)
            assert np.array_equal(np.signbit(u[u == 0.0]), np.signbit(ref[ref == 0.0])), (pc, n, v, scale)


@pytest.mark.parametrize("npts,levels,t", SHAPES)
@pytest.mark.parametrize("mesh", [0, 1, 2])
@pytest.mark.parametrize("pc", ["yline", "xline", "altline"])
def test_tail_equals_one_cycle_of_the_reference(mgk, orc, pc, mesh, npts, levels, t):
    view = _view(_hierarchy(orc, npts, levels, mesh, pc), t)
    tabs = _Tables(mgk, view.ct, uniform=(mesh == 0))
    try:
        _check(mgk, view, tabs, pc, 1000 * npts + 10 * mesh + t)
    finally:
        tabs.free()


@pytest.mark.parametrize("n0", [3, 15, 63])
@pytest.mark.parametrize("pc", ["yline", "xline", "altline"])
def test_non_symmetric_row_tables(mgk, orc, pc, n0):
    """S != N, W != E, varying with the row, on every level: a swapped neighbour, a transposed index or a reversed march shows (the reference
    changes under each of them on these tables: tests/test_xline_kernels_gpu.py)"""
    ns = [n0]
    while ns[-1] > 1:
        ns.append((ns[-1] - 1) // 2)
    rng = np.random.default_rng(77 + n0)
    h = XR.Hierarchy.__new__(XR.Hierarchy)
    h.orc, h.npts, h.levels, h.mesh, h.pc, h.log = orc, n0 + 2, len(ns), 1, pc, []
    h.n = ns
    h.ct = [distinct_row_tables(rng, n)[0] for n in ns]
    h.tab = [LR.tables(ct) for ct in h.ct]
    h.xg = [XR.table(ct) for ct in h.ct]
    tabs = _Tables(mgk, h.ct, uniform=False)
    try:
        _check(mgk, h, tabs, pc, 5000 + n0)
        # the reference itself tells the neighbours apart on these tables
        b = rng.uniform(-1, 1, (n0, n0))
        sw = copy.copy(h)
        sw.ct = [ct[:, [4, 3, 2, 1, 0]] for ct in h.ct]
        sw.log = []
        if n0 > 1:
            assert not np.array_equal(_reference(h, b, 0.8, (3, 3)), _reference(sw, b, 0.8, (3, 3)))
    finally:
        tabs.free()


def test_refusals(mgk, orc):
    """every refusal returns MGK_EINVAL and its message"""
    h = _view(_hierarchy(orc, 33, 5, 1, "altline"), 1)              # n = 15, 7, 3, 1
    tabs = _Tables(mgk, h.ct, uniform=False)
    g = mgk.geom(2, 15)
    db, du = _put(mgk, g, np.zeros((15, 15))), _put(mgk, g, None)
    big = mgk.geom(2, 127)
    dbig = mgk.field(big)
    g3 = mgk.geom(3, 15)

    def refused(msg, g0=g, n=h.n, pc=3, v=(3, 3), b=db, u=du, **over):
        a = tabs.args(pc)
        a.update(over)
        nl = len(n)
        if a["ctab"] is not None:
            a["ctab"] = a["ctab"][:nl] + [a["ctab"][-1]] * max(0, nl - len(a["ctab"]))
        for k in ("ltab", "gtab", "qtab", "xgtab", "xgs"):
            if a[k] is not None:
                a[k] = a[k][:nl] + [a[k][-1]] * max(0, nl - len(a[k]))
        rc = mgk.tail_cycle_line(g0, n, pc, scale=0.8, v=v, b=b, u=u, **a)
        with pytest.raises(Exception) as e:
            mgk._chk(rc)                                  # raises with the library's message
        err = str(e.value)
        assert rc == MGK_EINVAL and "mgk_tail_cycle_line_f64" in err and msg in err, (rc, err, msg)

    try:
        refused("2-D", g0=g3)
        refused("do not fit in LDS", g0=big, n=[127], pc=1, b=dbig, u=dbig)
        refused("whole square of n[0]", n=[7, 3, 1])
        refused("n[l-1] = 2 n[l] + 1", n=[15, 7, 2])
        refused("n[l-1] = 2 n[l] + 1", n=[15, 7, 3, 0])
        refused("1 to 8 levels", n=[15, 7, 3, 1, 1, 1, 1, 1, 1])
        refused("1 to 8 levels", v=(-1, 3))
        refused("1 to 8 levels", v=(3, -1))
        refused("1 to 8 levels", b=None)
        refused("1 to 8 levels", u=None)
        refused("1 to 8 levels", ctab=None)
        refused("pc must be", pc=0, ltab=None, gtab=None, qtab=None, xgtab=None, xgs=None)
        refused("pc must be", pc=4, ltab=None, gtab=None, qtab=None, xgtab=None, xgs=None)
        for pc in (1, 3):
            for k in ("ltab", "gtab", "qtab"):
                refused("the y sweeps need", pc=pc, **{k: None})
        for pc in (2, 3):
            refused("the x sweeps need", pc=pc, xgtab=None)
            refused("the x sweeps need", pc=pc, xgs=None)
        refused("null table of a level", pc=1, ltab=tabs.lt[:3] + [None])
        refused("null table of a level", pc=2, xgtab=[None] + tabs.xg[1:])
        refused("null table of a level", pc=3, ctab=tabs.ct[:2] + [None] + tabs.ct[3:])
        refused("row stride is 0 or at least n", pc=2, xgs=[14, 16, 16, 16])
        # what is allowed around them: y-line with no x tables at all, x-line with no y tables, and nothing was written by a refused call
        assert mgk.tail_cycle_line(g, h.n, 1, scale=0.8, v=(1, 1), b=db, u=du, ctab=tabs.ct, ltab=tabs.lt, gtab=tabs.gt, qtab=tabs.qt) == 0
        assert mgk.tail_cycle_line(g, h.n, 2, scale=0.8, v=(1, 1), b=db, u=du, ctab=tabs.ct, xgtab=tabs.xg, xgs=tabs.xgs) == 0
        mgk.sync()
        assert np.array_equal(_get(mgk, g, du), np.zeros((15, 15)))
    finally:
        tabs.free()
        for p in (db, du, dbig):
            mgk.free(p)
