"""The context's reduction scratch (mgk_ctx::partials: 3 rows of 16384 doubles, never cleared, shared by every reducing entry point) under test.

Every kernel that returns a sum of squares, a dot product or an error norm deposits per-block / per-wave partials there and a finishing kernel
adds up the `nparts` slots the launcher reports.  Three mistakes are invisible to a comparison of the returned sums when the same call ran
before on the same inputs (the tuning-variant loops of the kernel tests) or the scratch is fresh: a slot that is counted but not written (block
counts rounded up for the XCD tile order, whole waves or blocks without rows), a slot written beyond `nparts` or beyond the row (the refit and
refusal branches of the launchers, which the constant cap keeps out of reach of a test-sized shape), and the deferred half of finish_to_host.

Here every call runs through tests/guarded.py, which fills the WHOLE scratch with a NaN of known bits before each call of a REDUCERS entry, and
the scratch is downloaded after the call (mgk_debug_partials).  mgk_debug_set_max_partials lowers the cap every launcher reads, the allocation
staying what it is, so an overflow lands in poisoned, allocated memory and is a failed comparison, never an out-of-bounds store.

 a. default cap: the written slots are exactly a prefix [0, n) of each row the entry point uses (n = the nparts it reports, where it reports
    one), all finite (non-negative for sums of squares), math.fsum of them equals the returned value to RED_RTOL (max: exactly), every other
    slot keeps the poison bit for bit; under each tuning variant / z-chunk the entry point's own test loops over
 b. cap n - 1, then the largest cap under n / 4 that still holds one block per tile: VERDICT[launcher] says what the launcher does above its
    cap.  refits: success, at most cap slots per row, sum to RED_RTOL, output fields bit-identical to (a).  refuses: MGK_EINVAL naming the
    partial slots, outputs and scratch still entirely poison (nothing was launched)
 c. cap 1 where the shape has more than one tile: every launcher refuses
 d. the range forms (part_off): the three-range sequence of the solver; disjoint slot intervals written in full, the finish over their union;
    a cap that leaves too little room after part_off
 e. deferred results (mgk_defer_result) for every entry point that ends in finish_to_host with one slot; OWN_PROTOCOL lists the others
 f. one 2-D and one 3-D solve with the scratch poisoned before solve(): iterations, residual history and solution bit-identical

Shapes: per entry point the smallest shape of its case in tests/test_guarded_gpu.py that launches at least 4 blocks or waves, in each dispatch
form: 31^3 / 63^2 (k_stencil tiles), 511 x 27 x 9 and 1023 x 53 x 5 / 1023 x 51 x 5 (full-row 3-D forms), 255 x 255 x 5 (fp32 bridges), 119 / 121 wide (2-D and 3-D
wave forms).  References: tests/coef_cases.py np_sweep / np_residual and tests/rect_reference.py (the oracle's arithmetic restated in numpy: boxes
and row tables, held to the oracle by their own tests) and the oracle's long-double sumsq.  Sums to RED_RTOL = 1e-13 (tests/test_kernels_gpu.py),
fields bit for bit.  Two coefficient sets where a stencil is applied: the level's own (powers of two on 2^k - 1 wide grids: the exact-FMA
instances) and pairwise distinct ones.  tests/test_reduction_scratch_cpu.py holds the completeness gate and the dry run over the host stand-ins."""
import ctypes as C
import math

import numpy as np
import pytest

import rect_reference as RR
from cheby_reference import EIGS, cheb7
from coef_cases import dense_field, distinct_coef, distinct_row_tables, np_residual, np_sweep
from guarded import REDUCERS, Guarded, is_poison
from multigrid_petsc_amd.mgk import Geom
from oracle import Oracle

pytestmark = pytest.mark.gpu
RED_RTOL = 1e-13          # the project's figure for sums of squares (tests/test_kernels_gpu.py)
SCALE = 0.8
EINVAL = 10001            # MGK_EINVAL
SLOTS = 16384             # slots per row of the scratch
SENT = 4.25e77            # what the neighbours of a deferred slot hold


@pytest.fixture(scope="module")
def orc():
    return Oracle()


# what each launcher does when its block count exceeds the slot cap, from csrc/*.hip
VERDICT = {
    "launch_st": "refits",              # "fewer, longer chunks so that the partial buffer suffices"; fewer slots than tiles: refused
    "launch_jrow": "refits",            # the same rule on the register / shuffle sweep of the full rows
    "jacobi3_2d": "refits",             # longer chunks of rows, counted in whole blocks of four waves
    "jacobi3_3d_launch": "refits",      # fewer z chunks
    "flat_grid": "refits",              # mgk_flat_dot clamps its grid: the kernel strides over the vector
    "jacobi2": "refuses", "jacobi2_2d": "refuses", "jacobi3s": "refuses", "row_grid": "refuses", "kry_grid": "refuses",
}
# entry points whose result does not leave through finish_to_host with one slot: a pending mgk_defer_result must not reach them
OWN_PROTOCOL = {
    "mgk_error_sums_f64": "three values (max, sum, sum of squares) finished into result_dev[0 .. 2] and always delivered to the host",
    "mgk_multi_dot_f64": "k dot products finished into the caller's own device array out_dev, delivered at once or by mgk_krylov_fetch",
    "mgk_multi_axpy_sumsq_f64": "finishes into result_dev[MGK_KRYLOV_MAX]; NULL for sumsq_host defers to mgk_krylov_fetch, its own protocol",
}


def _sumsq(orc, x):
    return orc.sumsq(np.ascontiguousarray(x, dtype=np.float64).ravel())


def _geom32(G, nx, ny, nz):
    g = Geom()
    G._chk(G.L.mgk_geom_init_f32(C.byref(g), 3, nx, ny, nz))
    return g


def _cdiv(a, b):
    return -(-a // b)


def _late(L, name):
    """L.name, looked up when it is called (a host stand-in library may lack it: the op can still be built and asked for its tables)"""
    return lambda *a: getattr(L, name)(*a)


# ------------------------------------------------------------------------------------------------------------------------------
# a problem on a box, and one reducing call on it
# ------------------------------------------------------------------------------------------------------------------------------
class Box:
    """seeded dense fields u, b on an nx x ny (x nz) grid on the device and the host; kind: 'level' (the stencil of the uniform level with
    nx unknowns per side) or 'distinct' (pairwise distinct coefficients)"""

    def __init__(self, G, dim, nx, ny, nz, kind):
        rng = np.random.default_rng([51000, dim, nx, ny, nz, kind == "level"])
        self.G, self.dim, self.nx, self.ny, self.nz = G, dim, nx, ny, nz
        self.shape = (nz, ny, nx) if dim == 3 else (ny, nx)
        q = float((nx + 1) ** 2)
        level = [q, q, q, -6.0 * q, q, q, q] if dim == 3 else [q, q, -4.0 * q, q, q]
        self.As = np.array(level) if kind == "level" else distinct_coef(rng, dim)
        self.dinv = 1.0 / float(self.As[self.As.size // 2])
        self.rng = rng
        self.u, self.b = dense_field(rng, *self.shape), dense_field(rng, *self.shape)
        self.g = G.geom(dim, nx, ny, nz if dim == 3 else 1)
        self.gp, self.coef = C.byref(self.g), G.coef(list(self.As))
        self.own = []
        self.du, self.db = self.to(self.u), self.to(self.b)
        if dim == 2:                     # row tables: the constant stencil as a table ('level') or a set per row ('distinct')
            self.ct, self.dt = RR.const_table(self.As, ny) if kind == "level" else distinct_row_tables(rng, ny)

    def to(self, x):
        p = self.G.to_field(self.g, np.asarray(x).ravel())
        self.own.append(p)
        return p

    def up(self, x):
        p = self.G.upload(np.asarray(x, dtype=np.float64).ravel())
        self.own.append(p)
        return p

    def out(self):
        p = self.G.field(self.g)
        self.own.append(p)
        return p

    def J(self, x):
        return np_sweep(self.As, SCALE, self.b, x)

    def res(self, x):
        return np_residual(self.As, self.b, x)

    def close(self):
        for p in self.own:
            self.G.free(p)
        self.own = []


class Op:
    """one reducing call.  call(): runs it through the proxy and returns the return code; values: what it delivered to the host; nparts: the
    count it reported (None: it reports none).  want: the reference values; kinds: per value 'sumsq' | 'sum' | 'max' | 'dot'; outs: the output
    fields (geometry, pointer, reference, dtype); rows(cap): where the rows of partials start; packed: the values' partials lie one after
    the other in ONE run of slots (mgk_multi_dot_f64); cap_rows: rows of `cap` slots the launcher may fill; min_cap: the smallest cap under
    which the launcher still launches (its tiles), None: any cap under n is refused"""

    def __init__(self, P, name, launcher, invoke, want, outs=(), kinds=None, nvals=1, rows=None, packed=False, cap_rows=1, min_cap=None, reports=False,
                 prepare=None, deferrable=True):
        self.P, self.name, self.launcher, self.invoke, self.outs = P, name, launcher, invoke, list(outs)
        self.want = [float(w) for w in want]
        self.kinds = kinds or ["sumsq"] * len(self.want)
        self.nvals, self.rows, self.packed, self.cap_rows, self.min_cap, self.reports = nvals, rows or (lambda cap: [0]), packed, cap_rows, min_cap, reports
        self.prepare, self.deferrable = prepare, deferrable
        self.values, self.nparts = None, None

    def call(self):
        if self.prepare:
            self.prepare()
        host = (C.c_double * self.nvals)(*([-1.0] * self.nvals))
        nparts = C.c_int(-1)
        rc = self.invoke(host, nparts)
        self.values = list(host)
        self.nparts = nparts.value if self.reports else None
        return rc


def _coarse_tiles(dim, nx, ny, resnorm=False):
    """tiles of launch_st under the default variant of dispatch_st<fp64>: (columns per tile, rows per tile) by nx"""
    if dim == 2:
        tx = 512 if nx >= 511 else 256 if nx >= 255 else 128
        return _cdiv(nx + 1, tx)
    if resnorm and nx >= 255:
        tx, ty = 256, 8
    elif nx >= 1023:
        tx, ty = 1024, 4
    elif nx >= 511:
        tx, ty = 512, 4
    elif nx >= 255:
        tx, ty = 256, 4
    elif nx >= 127:
        tx, ty = 128, 8
    else:
        tx, ty = 128, 4
    return _cdiv(nx + 1, tx) * _cdiv(ny, ty)


def _st_or_jrow(P):
    """(launcher, min_cap) of the plain sweep with a norm: the register form takes the full rows of 1024 by default, k_stencil the rest"""
    if P.dim == 3 and P.nx + 1 == 1024 and (P.ny + 1) % 4 == 0:
        return "launch_jrow", _cdiv(P.ny, 4)
    return "launch_st", _coarse_tiles(P.dim, P.nx, P.ny)


def _wave_tiles_2d(P):
    return 4 * _cdiv(_cdiv((P.nx + 1) // 2, 60), 4)              # whole blocks of four waves


# ---- the builders: name -> function(P) -> Op ----------------------------------------------------------------------------------
def _b_residual_sumsq(P):
    L, G = P.G.L, P.G
    return Op(P, "mgk_residual_sumsq_f64", "launch_st", lambda h, n: L.mgk_residual_sumsq_f64(G.ctx, P.gp, P.coef, P.db, P.du, h, None),
              [_sumsq(P.orc, P.res(P.u))], min_cap=_coarse_tiles(P.dim, P.nx, P.ny, resnorm=True))


def _b_jacobi_sumsq(P):
    L, G, o = P.G.L, P.G, P.out()
    launcher, mc = _st_or_jrow(P)
    return Op(P, "mgk_jacobi_sumsq_f64", launcher, lambda h, n: L.mgk_jacobi_sumsq_f64(G.ctx, P.gp, P.coef, P.dinv, SCALE, P.db, P.du, o, h, None),
              [_sumsq(P.orc, P.res(P.u))], [(P.g, o, P.J(P.u), np.float64)], min_cap=mc)


def _b_jacobi_sumsq_store(P):
    L, G, o, r = P.G.L, P.G, P.out(), P.out()
    return Op(P, "mgk_jacobi_sumsq_store_f64", "launch_st",
              lambda h, n: L.mgk_jacobi_sumsq_store_f64(G.ctx, P.gp, P.coef, P.dinv, SCALE, None, None, P.db, P.du, o, r, h, None),
              [_sumsq(P.orc, P.res(P.u))], [(P.g, o, P.J(P.u), np.float64), (P.g, r, P.res(P.u), np.float64)], min_cap=_coarse_tiles(2, P.nx, P.ny))


def _ranged(P, name, launcher, one, want, outs, min_cap):
    """a range form over the whole marching axis in one call at part_off 0, closed by mgk_partials_finish"""
    L, G = P.G.L, P.G

    def invoke(h, n):
        rc = one(0, P.nz if P.dim == 3 else P.ny, 0, n)
        return rc if rc else L.mgk_partials_finish(G.ctx, n.value, h, None)
    return Op(P, name, launcher, invoke, want, outs, min_cap=min_cap, reports=True)


def _range_call(P, name, o):
    L, G = P.G.L, P.G
    if name == "mgk_jacobi_sumsq_range_f64":
        return lambda z0, z1, off, n: L.mgk_jacobi_sumsq_range_f64(G.ctx, P.gp, P.coef, P.dinv, SCALE, P.db, P.du, o, z0, z1, off, C.byref(n), None)
    fn = _late(L, name)
    return lambda z0, z1, off, n: fn(G.ctx, P.gp, None, P.coef, P.dinv, SCALE, P.db, P.du, o, None, 0, 0, z0, z1, off, C.byref(n), None)


def _b_jacobi_sumsq_range(P):
    o = P.out()
    launcher, mc = _st_or_jrow(P)
    return _ranged(P, "mgk_jacobi_sumsq_range_f64", launcher, _range_call(P, "mgk_jacobi_sumsq_range_f64", o), [_sumsq(P.orc, P.res(P.u))],
                   [(P.g, o, P.J(P.u), np.float64)], mc)


def _two(P, name, mid, ranged):
    L, G, o = P.G.L, P.G, P.out()
    j1 = P.J(P.u)
    want, outs = [_sumsq(P.orc, P.res(j1 if mid else P.u))], [(P.g, o, P.J(j1), np.float64)]
    if ranged:
        return _ranged(P, name, "jacobi2", _range_call(P, name, o), want, outs, None)
    fn = _late(L, name)
    return Op(P, name, "jacobi2", lambda h, n: fn(G.ctx, P.gp, P.coef, P.dinv, SCALE, P.db, P.du, o, h, None), want, outs)


def _b_jacobi2_2d_sumsq(P):
    L, G, o = P.G.L, P.G, P.out()
    return Op(P, "mgk_jacobi2_2d_sumsq_f64", "jacobi2_2d", lambda h, n: L.mgk_jacobi2_2d_sumsq_f64(G.ctx, P.gp, P.coef, P.dinv, SCALE, P.db, P.du, o, h, None),
              [_sumsq(P.orc, P.res(P.u))], [(P.g, o, P.J(P.J(P.u)), np.float64)])


def _tables(P):
    return P.up(P.ct), P.up(P.dt)


def _rt_sweep(P, x):
    return RR.sweep(P.ct, P.dt, SCALE, P.b, x)


def _b_jacobi2_2d_sumsq_rowcoef(P):
    L, G, o = P.G.L, P.G, P.out()
    dct, ddt = _tables(P)
    return Op(P, "mgk_jacobi2_2d_sumsq_rowcoef_f64", "jacobi2_2d", lambda h, n: L.mgk_jacobi2_2d_sumsq_rowcoef_f64(G.ctx, P.gp, dct, ddt, SCALE, P.db, P.du, o, h, None),
              [_sumsq(P.orc, RR.residual(P.ct, P.b, P.u))], [(P.g, o, _rt_sweep(P, _rt_sweep(P, P.u)), np.float64)])


def _b_jacobi_sumsq_rowcoef(P):
    L, G, o = P.G.L, P.G, P.out()
    dct, ddt = _tables(P)
    return Op(P, "mgk_jacobi_sumsq_rowcoef_f64", "launch_st", lambda h, n: L.mgk_jacobi_sumsq_rowcoef_f64(G.ctx, P.gp, dct, ddt, SCALE, P.db, P.du, o, h, None),
              [_sumsq(P.orc, RR.residual(P.ct, P.b, P.u))], [(P.g, o, _rt_sweep(P, P.u), np.float64)], min_cap=_coarse_tiles(2, P.nx, P.ny))


def _b_residual_sumsq_rowcoef(P):
    L, G = P.G.L, P.G
    dct, _ = _tables(P)
    return Op(P, "mgk_residual_sumsq_rowcoef_f64", "launch_st", lambda h, n: L.mgk_residual_sumsq_rowcoef_f64(G.ctx, P.gp, dct, P.db, P.du, h, None),
              [_sumsq(P.orc, RR.residual(P.ct, P.b, P.u))], min_cap=_coarse_tiles(2, P.nx, P.ny, resnorm=True))


def _b_sumsq(P):
    L, G = P.G.L, P.G
    return Op(P, "mgk_sumsq_f64", "row_grid", lambda h, n: L.mgk_sumsq_f64(G.ctx, P.gp, P.db, h, None), [_sumsq(P.orc, P.b)])


def _b_error_sums(P):
    L, G = P.G.L, P.G
    sx, sy, sz = (dense_field(P.rng, m) for m in (P.nx, P.ny, P.nz))
    sol = sx[None, :] * sy[:, None]
    if P.dim == 3:
        sol = sol[None, :, :] * sz[:, None, None]
    d = np.abs(P.u - sol)
    dsx, dsy, dsz = P.up(sx), P.up(sy), P.up(sz)
    return Op(P, "mgk_error_sums_f64", "row_grid", lambda h, n: L.mgk_error_sums_f64(G.ctx, P.gp, P.du, dsx, dsy, dsz, h, None),
              [d.max(), math.fsum(d.ravel()), math.fsum((d * d).ravel())], kinds=["max", "sum", "sumsq"], nvals=3, rows=lambda cap: [0, cap, 2 * cap],
              deferrable=False)


def _b_flat_dot(P):
    L, G = P.G.L, P.G
    n = P.nx * P.ny
    x = P.u.ravel()
    y = P.b.ravel() + 0.5 * x            # (correlated, as the basis fields of tests/test_gmres_kernels_gpu.py: the dot product does not cancel)
    dx, dy = P.up(x), P.up(y)
    return Op(P, "mgk_flat_dot", "flat_grid", lambda h, m: L.mgk_flat_dot(G.ctx, n, dx, dy, h, None), [math.fsum(x * y)], kinds=["dot"], min_cap=1)


def _bridge(P, name, corrected, jz):
    L, G = P.G.L, P.G
    g32 = _geom32(G, P.nx, P.ny, P.nz)
    r32, e0, un = G.field32(g32), G.field32(g32), P.out()
    P.own += [r32, e0]
    e = dense_field(P.rng, *P.shape).astype(np.float32)
    de = G.to_field32(g32, e.ravel())
    P.own.append(de)
    ucorr = P.u + e.astype(np.float64)
    r = P.res(ucorr if corrected else P.u)
    rr = r.astype(np.float32)
    outs = [(g32, r32, rr, np.float32)]
    if corrected:
        outs.append((P.g, un, ucorr, np.float64))
    if jz:
        outs.append((g32, e0, np.float32(SCALE) * (rr * np.float32(P.dinv)), np.float32))
    g32p = C.byref(g32)
    fn = _late(L, name)
    if corrected and jz:
        inv = lambda h, n: fn(G.ctx, P.gp, g32p, P.coef, P.db, P.du, de, un, r32, e0, P.dinv, SCALE, h, None)
    elif corrected:
        inv = lambda h, n: fn(G.ctx, P.gp, g32p, P.coef, P.db, P.du, de, un, r32, h, None)
    elif jz:
        inv = lambda h, n: fn(G.ctx, P.gp, g32p, P.coef, P.db, P.du, r32, e0, P.dinv, SCALE, h, None)
    else:
        inv = lambda h, n: fn(G.ctx, P.gp, g32p, P.coef, P.db, P.du, r32, h, None)
    op = Op(P, name, "launch_st", inv, [_sumsq(P.orc, r)], outs, min_cap=_coarse_tiles(3, P.nx, P.ny))
    op.keep = g32
    return op


def _three_2d(P, name, store=False, cheb=False):
    L, G, o = P.G.L, P.G, P.out()
    fn = _late(L, name)
    outs = []
    if cheb:
        c7 = cheb7(*EIGS[1])
        c7p = c7.ctypes.data_as(C.POINTER(C.c_double))
        ct, dt = RR.const_table(P.As, P.ny)
        outs.append((P.g, o, RR.cheby3(ct, dt, c7, P.b, P.u), np.float64))
        inv = lambda h, n: fn(G.ctx, P.gp, P.coef, P.dinv, c7p, None, None, P.db, P.du, o, h, None)
    else:
        outs.append((P.g, o, P.J(P.J(P.J(P.u))), np.float64))
        if store:
            r = P.out()
            outs.append((P.g, r, P.res(P.u), np.float64))
            inv = lambda h, n: fn(G.ctx, P.gp, P.coef, P.dinv, SCALE, None, None, P.db, P.du, o, r, h, None)
        else:
            inv = lambda h, n: fn(G.ctx, P.gp, P.coef, P.dinv, SCALE, None, None, P.db, P.du, o, h, None)
    op = Op(P, name, "jacobi3_2d", inv, [_sumsq(P.orc, P.res(P.u))], outs, min_cap=_wave_tiles_2d(P))
    op.keep = locals().get("c7")
    return op


def _three_3d(P, name, mid):
    L, G, o = P.G.L, P.G, P.out()
    fn = _late(L, name)
    j1 = P.J(P.u)
    stacked = P.nx + 1 in (512, 1024)
    if stacked:
        launcher, mc = "jacobi3s", None
    else:                                # one partial per wave, four waves per block; a wave tile holds 120 columns x 3 rows with the norm
        launcher, mc = "jacobi3_3d_launch", 4 * _cdiv(_cdiv((P.nx + 1) // 2, 60) * _cdiv(P.ny, 3), 4)
    return Op(P, name, launcher, lambda h, n: fn(G.ctx, P.gp, P.coef, P.dinv, SCALE, P.db, P.du, o, h, None),
              [_sumsq(P.orc, P.res(j1 if mid else P.u))], [(P.g, o, P.J(P.J(j1)), np.float64)], min_cap=mc)


KRY_K = 7


def _krylov(P, axpy):
    L, G = P.G.L, P.G
    w = P.u
    v = [dense_field(P.rng, *P.shape) + 0.5 * w for _ in range(KRY_K)]
    dv = [P.to(x) for x in v]
    ptrs = (C.c_void_p * KRY_K)(*[p.value for p in dv])
    if not axpy:
        hdev = P.up(np.full(KRY_K, SENT))
        op = Op(P, "mgk_multi_dot_f64", "kry_grid", lambda h, n: L.mgk_multi_dot_f64(G.ctx, P.gp, KRY_K, ptrs, P.du, hdev, h, None),
                [math.fsum((x * w).ravel()) for x in v], kinds=["dot"] * KRY_K, nvals=KRY_K, packed=True, cap_rows=3, deferrable=False)
        op.keep = (ptrs, hdev)
        return op
    h = P.rng.uniform(-0.5, 0.5, KRY_K)
    hdev = P.up(h)
    ref = w.copy()
    for i in range(KRY_K):
        ref = ref - h[i] * v[i]
    state = {}

    def prepare():                       # w is input and output at once: a fresh copy for every call
        state["w"] = P.to(w)
        op.outs = [(P.g, state["w"], ref, np.float64)]
    op = Op(P, "mgk_multi_axpy_sumsq_f64", "kry_grid", lambda hh, n: L.mgk_multi_axpy_sumsq_f64(G.ctx, P.gp, KRY_K, hdev, ptrs, state["w"], hh, None),
            [math.fsum((ref * ref).ravel())], prepare=prepare, deferrable=False)
    op.keep, op.in_place = (ptrs, hdev), w
    return op


BUILDERS = {
    "mgk_residual_sumsq_f64": _b_residual_sumsq,
    "mgk_jacobi_sumsq_f64": _b_jacobi_sumsq,
    "mgk_jacobi_sumsq_store_f64": _b_jacobi_sumsq_store,
    "mgk_jacobi_sumsq_range_f64": _b_jacobi_sumsq_range,
    "mgk_jacobi2_sumsq_f64": lambda P: _two(P, "mgk_jacobi2_sumsq_f64", False, False),
    "mgk_jacobi2_sumsq_mid_f64": lambda P: _two(P, "mgk_jacobi2_sumsq_mid_f64", True, False),
    "mgk_jacobi2_sumsq_slab_f64": lambda P: _two(P, "mgk_jacobi2_sumsq_slab_f64", False, True),
    "mgk_jacobi2_sumsq_mid_slab_f64": lambda P: _two(P, "mgk_jacobi2_sumsq_mid_slab_f64", True, True),
    "mgk_jacobi2_2d_sumsq_f64": _b_jacobi2_2d_sumsq,
    "mgk_jacobi2_2d_sumsq_rowcoef_f64": _b_jacobi2_2d_sumsq_rowcoef,
    "mgk_sumsq_f64": _b_sumsq,
    "mgk_error_sums_f64": _b_error_sums,
    "mgk_flat_dot": _b_flat_dot,
    "mgk_residual_f64_to_f32": lambda P: _bridge(P, "mgk_residual_f64_to_f32", False, False),
    "mgk_residual_f64_to_f32_jz": lambda P: _bridge(P, "mgk_residual_f64_to_f32_jz", False, True),
    "mgk_correct_residual_f64_f32": lambda P: _bridge(P, "mgk_correct_residual_f64_f32", True, False),
    "mgk_correct_residual_f64_f32_jz": lambda P: _bridge(P, "mgk_correct_residual_f64_f32_jz", True, True),
    "mgk_jacobi_sumsq_rowcoef_f64": _b_jacobi_sumsq_rowcoef,
    "mgk_residual_sumsq_rowcoef_f64": _b_residual_sumsq_rowcoef,
    "mgk_jacobi3_2d_sumsq_f64": lambda P: _three_2d(P, "mgk_jacobi3_2d_sumsq_f64"),
    "mgk_jacobi3_2d_sumsq_store_f64": lambda P: _three_2d(P, "mgk_jacobi3_2d_sumsq_store_f64", store=True),
    "mgk_cheby3_2d_sumsq_f64": lambda P: _three_2d(P, "mgk_cheby3_2d_sumsq_f64", cheb=True),
    "mgk_jacobi3_sumsq_f64": lambda P: _three_3d(P, "mgk_jacobi3_sumsq_f64", False),
    "mgk_jacobi3_sumsq_mid_f64": lambda P: _three_3d(P, "mgk_jacobi3_sumsq_mid_f64", True),
    "mgk_multi_dot_f64": lambda P: _krylov(P, False),
    "mgk_multi_axpy_sumsq_f64": lambda P: _krylov(P, True),
}

# ---- shapes and the tuning variants of each entry point's own test -------------------------------------------------------------
CUBE, SQUARE, ROW512, ROW1024, WIDE32 = (3, 31, 31, 31), (2, 63, 63, 1), (3, 511, 27, 9), (3, 1023, 53, 5), (3, 255, 255, 5)
ROW1024J = (3, 1023, 51, 5)           # (the row sweeps and the two-sweep passes take their register forms where ny + 1 is a multiple of 4)
W119, W121 = (2, 119, 119, 1), (2, 121, 121, 1)
PLAIN = ((-1, -1),)
ZC4 = ((-1, -1), (-1, 4))                                                        # tests/test_headline_width_gpu.py
ZC5 = ((-1, -1), (-1, 5))                                                        # tests/test_kernels_gpu.py
J3_2D = ((-1, -1), (50, -1), (51, -1), (52, -1), (-1, 1), (-1, 5), (-1, 12), (-1, 64), (58, -1), (58, 5), (58, 12), (57, -1), (59, -1), (59, 5),
         (53, -1), (54, -1), (54, 5), (60, -1), (61, -1))                       # tests/test_three_sweeps_gpu.py
J3_STORE = ((-1, -1), (50, -1), (51, -1), (52, -1))
CH3 = ((-1, -1), (50, -1), (51, -1), (52, -1), (-1, 1), (-1, 5), (-1, 64), (58, 12), (59, 5))      # tests/test_cheby3_kernels_gpu.py
J3_3D = ((-1, -1), (62, -1), (63, -1), (64, -1), (-1, 1), (-1, 5), (63, 7), (53, 16))
STACKED = ((-1, -1), (67, -1), (67, 1), (67, 2), (67, 5), (68, -1), (68, 2), (65, -1), (65, 2))      # tests/test_triple_mid_gpu.py
MID = ((-1, -1), (-1, 1), (-1, 2), (-1, 5), (68, -1), (68, 5), (65, -1), (65, 1))
BRIDGE = ((-1, -1), (-1, 3))                                                     # tests/test_mixed_width_gpu.py
KRY = ((-1, -1), (0, -1), (1, -1))                                               # tests/test_gmres_kernels_gpu.py: the store policies
# entry point -> [(shape, variants of (a), tuning of (b) / (c))]
SHAPES = {
    "mgk_residual_sumsq_f64": [(CUBE, ZC5, None), (SQUARE, ZC5, None), (ROW512, ZC4, None)],
    "mgk_jacobi_sumsq_f64": [(CUBE, ZC5 + ((2, -1), (2, 5)), None), (SQUARE, ZC5 + ((0, 5),), None), (ROW512, ZC4 + ((34, -1),), None), (ROW1024J, ZC4, None)],
    "mgk_jacobi_sumsq_store_f64": [(SQUARE, PLAIN, None), ((2, 255, 255, 1), PLAIN, None)],
    "mgk_jacobi_sumsq_range_f64": [(CUBE, ((-1, -1), (0, -1)), None), ((2, 255, 255, 1), PLAIN, None), (ROW1024J, PLAIN, None)],
    "mgk_jacobi2_sumsq_f64": [(ROW512, ZC4, None), (ROW1024J, ZC4, None)],
    "mgk_jacobi2_sumsq_mid_f64": [(ROW512, ZC4, None), (ROW1024J, ZC4, None)],
    "mgk_jacobi2_sumsq_slab_f64": [(ROW512, ZC4, None), (ROW1024J, PLAIN, None)],
    "mgk_jacobi2_sumsq_mid_slab_f64": [(ROW512, ZC4, None), (ROW1024J, PLAIN, None)],
    "mgk_jacobi2_2d_sumsq_f64": [((2, 127, 127, 1), PLAIN, None), ((2, 243, 243, 1), PLAIN, None)],
    "mgk_jacobi2_2d_sumsq_rowcoef_f64": [(SQUARE, PLAIN, None), ((2, 243, 243, 1), PLAIN, None)],
    "mgk_sumsq_f64": [(CUBE, PLAIN, None), (SQUARE, PLAIN, None), (ROW512, ZC4, None)],
    "mgk_error_sums_f64": [((2, 31, 31, 1), PLAIN, None), ((3, 15, 15, 15), PLAIN, None)],
    "mgk_flat_dot": [((2, 257, 9, 1), PLAIN, None)],
    "mgk_residual_f64_to_f32": [(CUBE, BRIDGE, None), (WIDE32, BRIDGE, None)],
    "mgk_residual_f64_to_f32_jz": [(CUBE, BRIDGE, None), (WIDE32, BRIDGE, None)],
    "mgk_correct_residual_f64_f32": [(CUBE, BRIDGE + ((2, 3),), None), (WIDE32, BRIDGE, None)],
    "mgk_correct_residual_f64_f32_jz": [(CUBE, BRIDGE, None), (WIDE32, BRIDGE, None)],
    "mgk_jacobi_sumsq_rowcoef_f64": [(SQUARE, PLAIN, None), ((2, 255, 255, 1), PLAIN, None)],
    "mgk_residual_sumsq_rowcoef_f64": [(SQUARE, PLAIN, None), ((2, 255, 255, 1), PLAIN, None)],
    "mgk_jacobi3_2d_sumsq_f64": [(W119, J3_2D, None), (W121, J3_2D, None)],
    "mgk_jacobi3_2d_sumsq_store_f64": [(W119, J3_STORE, None), ((2, 255, 255, 1), J3_STORE, None)],
    "mgk_cheby3_2d_sumsq_f64": [(W121, CH3, None), ((2, 239, 239, 1), CH3, None)],
    # (b) of the independent-wave form under z chunks of one plane: by default these thin grids are one chunk, and the refit cuts chunks
    "mgk_jacobi3_sumsq_f64": [((3, 119, 9, 11), J3_3D, (-1, 1)), ((3, 121, 5, 7), J3_3D, (-1, 1)), (ROW512, STACKED, None), (ROW1024, STACKED, None)],
    "mgk_jacobi3_sumsq_mid_f64": [(ROW512, MID, None), (ROW1024, MID, None)],
    "mgk_multi_dot_f64": [((2, 127, 127, 1), KRY, None), (CUBE, KRY, None)],
    "mgk_multi_axpy_sumsq_f64": [((2, 127, 127, 1), KRY, None), (CUBE, KRY, None)],
}
NO_STENCIL = {"mgk_sumsq_f64", "mgk_error_sums_f64", "mgk_flat_dot", "mgk_multi_dot_f64", "mgk_multi_axpy_sumsq_f64"}      # one coefficient set is enough
RANGE_FORMS = {"mgk_jacobi_sumsq_range_f64": ((1, -1), (0, 1), (-1, None)),                 # the solver's sequences (csrc/mg_solver.c): inner planes first
               "mgk_jacobi2_sumsq_slab_f64": ((2, -2), (0, 2), (-2, None)),
               "mgk_jacobi2_sumsq_mid_slab_f64": ((2, -2), (0, 2), (-2, None))}


def _sid(shape):
    return "x".join(map(str, shape[1:1 + shape[0]]))


def _cases(kinds=True):
    out = []
    for name, shapes in SHAPES.items():
        for shape, variants, cap_tuning in shapes:
            for kind in (("level",) if name in NO_STENCIL or not kinds else ("level", "distinct")):
                out.append(pytest.param(name, shape, variants, cap_tuning, kind, id=f"{name}-{_sid(shape)}-{kind}"))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the checks
# ------------------------------------------------------------------------------------------------------------------------------
def _close(got, want):
    return abs(got - want) <= RED_RTOL * abs(want)


def check_scratch(G, op, cap, host=False):
    """the scratch after a successful call of op under the slot cap `cap`: the written slots are exactly a prefix of each row; returns its length"""
    s = G.read_scratch()
    wr = ~is_poison(s)
    lens = []
    for st in op.rows(cap):
        run = wr[st:]
        lens.append(run.size if run.all() else int(np.argmin(run)))
    assert int(wr.sum()) == sum(lens), (f"{op.name}: slots outside the prefixes of the rows {op.rows(cap)} (lengths {lens}) were written: "
                                        f"{[int(q) for q in np.flatnonzero(wr)[:6]]} ... {[int(q) for q in np.flatnonzero(wr)[-6:]]}")
    assert len(set(lens)) == 1, f"{op.name}: the rows hold different numbers of partials: {lens}"
    n = lens[0]
    if host and n == 0:
        return 0                         # the host stand-ins reduce on the host
    assert 1 <= n <= cap * op.cap_rows, f"{op.name}: {n} slots written under a cap of {cap} x {op.cap_rows}"
    if op.nparts is not None:
        assert n == op.nparts, f"{op.name}: {n} slots written, {op.nparts} reported"
    if op.packed:
        assert n % op.nvals == 0, f"{op.name}: {n} slots for {op.nvals} values"
        m = n // op.nvals
        rows = [s[q * m:(q + 1) * m] for q in range(op.nvals)]
    else:
        rows = [s[st:st + n] for st in op.rows(cap)]
    for q, (row, kind, got) in enumerate(zip(rows, op.kinds, op.values)):
        assert np.all(np.isfinite(row)), f"{op.name}: value {q}: a partial is not finite"
        if kind != "dot":
            assert np.all(row >= 0.0), f"{op.name}: value {q}: a negative partial of a {kind}"
        if kind == "max":
            assert row.max() == got, f"{op.name}: the max of the partials {row.max()!r} is not the value returned {got!r}"
        else:
            tot = math.fsum(row)
            scale = abs(tot) if kind != "dot" else math.fsum(np.abs(row))
            assert abs(tot - got) <= RED_RTOL * scale, f"{op.name}: value {q}: fsum of the {n} partials {tot!r}, returned {got!r}"
    return n


def check_values(op):
    for q, (got, want, kind) in enumerate(zip(op.values, op.want, op.kinds)):
        if kind == "max":
            assert got == want, f"{op.name}: max {got!r} vs {want!r}"
        else:
            assert math.isfinite(got) and _close(got, want), f"{op.name}: value {q}: {got!r} vs the reference {want!r} (rel {abs(got - want) / abs(want):.2e})"


def fetch_outs(G, op):
    return [(G.from_field32 if dt == np.float32 else G.from_field)(g, p) for g, p, _, dt in op.outs]


def check_outs(op, got, tag):
    for q, (have, (_, _, want, dt)) in enumerate(zip(got, op.outs)):
        want = np.asarray(want, dtype=dt).ravel()
        assert np.array_equal(have, want), f"{op.name} {tag}: output {q}: {np.count_nonzero(have != want)} of {want.size} cells differ, {np.count_nonzero(np.isnan(have))} NaN"


def run_ok(G, op, cap, tag, host=False):
    rc = op.call()
    assert rc == 0, f"{op.name} {tag}: rc {rc}: {G.last_error()}"
    n = check_scratch(G, op, cap, host)
    check_values(op)
    got = fetch_outs(G, op)
    check_outs(op, got, tag)
    return n, got


def run_refused(G, op, tag):
    rc = op.call()
    msg = G.last_error()
    assert rc == EINVAL, f"{op.name} {tag}: rc {rc} ({msg}), expected a refusal"
    assert "partial" in msg and "slot" in msg, f"{op.name} {tag}: the refusal does not name the partial slots: {msg!r}"
    assert np.all(is_poison(G.read_scratch())), f"{op.name} {tag}: refused, yet the scratch was written"
    if getattr(op, "in_place", None) is not None:
        assert np.array_equal(fetch_outs(G, op)[0], op.in_place.ravel()), f"{op.name} {tag}: refused, yet w was changed"
    else:
        for q, have in enumerate(fetch_outs(G, op)):
            assert np.all(is_poison(have)), f"{op.name} {tag}: refused, yet output {q} was written"


class capped:
    """the slot cap lowered for the body, restored on the way out"""

    def __init__(self, G, cap):
        self.G, self.cap = G, cap

    def __enter__(self):
        self.G._chk(self.G.L.mgk_debug_set_max_partials(self.G.ctx, self.cap))

    def __exit__(self, *exc):
        self.G.L.mgk_debug_set_max_partials(self.G.ctx, 0)


def _session(mgk, orc, name, shape, kind):
    G = Guarded(mgk)
    P = Box(G, *shape, kind)
    P.orc = orc
    return G, P, BUILDERS[name](P)


def _finish(G, P, name):
    try:
        P.close()
        G.assert_no_leaks()
        assert G.scratch_poisoned_calls.get(name, 0) >= 1, f"the proxy never poisoned the scratch before {name}"
    finally:
        G.release()
        G.L.mgk_set_tuning(-1, -1)
        G.L.mgk_debug_set_max_partials(G.ctx, 0)


# ---- a. default cap -------------------------------------------------------------------------------------------------------------
def body_default_cap(mgk, orc, name, shape, variants, kind, host=False):
    G, P, op = _session(mgk, orc, name, shape, kind)
    try:
        ns = {}
        for var, zc in variants:
            G.L.mgk_set_tuning(var, zc)
            ns[(var, zc)], _ = run_ok(G, op, SLOTS, f"variant={var} zc={zc}", host)
        G.L.mgk_set_tuning(-1, -1)
        assert host or ns[(-1, -1)] >= 4, f"{name} on {shape}: only {ns[(-1, -1)]} blocks or waves: the shape is too small to be a case"
        assert G.scratch_poisoned_calls[name] == len(variants)
        assert np.array_equal(G.from_field(P.g, P.db), P.b.ravel()), "b was modified"
    except BaseException:
        G.release()
        G.L.mgk_set_tuning(-1, -1)
        raise
    _finish(G, P, name)
    return ns


@pytest.mark.parametrize("name,shape,variants,cap_tuning,kind", _cases())
def test_partials_are_a_prefix_under_the_default_cap(mgk, orc, name, shape, variants, cap_tuning, kind):
    body_default_cap(mgk, orc, name, shape, variants, kind)


# ---- b, c. lowered caps -----------------------------------------------------------------------------------------------------------
def body_lowered_caps(mgk, orc, name, shape, cap_tuning, kind="level"):
    G, P, op = _session(mgk, orc, name, shape, kind)
    try:
        G.L.mgk_set_tuning(*(cap_tuning or (-1, -1)))
        n, base = run_ok(G, op, SLOTS, "default cap")
        refits = VERDICT[op.launcher] == "refits"
        assert refits == (op.min_cap is not None)
        rows = op.cap_rows
        # n - 1; the largest cap under n / 4 that holds one block per tile (none where the tiles are a quarter of the blocks or more); cap 1
        caps = [(n - 1) // rows]
        quarter = (_cdiv(n, 4) - 1) // rows
        if quarter >= (op.min_cap or 1) and quarter >= 1:
            caps.append(quarter)
        if (op.min_cap or n) > 1:
            caps.append(1)
        if rows > 1:
            caps.insert(0, _cdiv(n, rows))       # (rows of the scratch filled to the brim: the launch fits and is the same launch)
        seen = set()
        for cap in caps:
            if cap < 1 or cap in seen:
                continue
            seen.add(cap)
            with capped(G, cap):
                if cap * rows >= n or (refits and cap >= op.min_cap):
                    m, got = run_ok(G, op, cap, f"cap={cap}")
                    assert m <= cap * rows
                    check_outs(op, got, f"cap={cap}")
                    for q, (a, b) in enumerate(zip(got, base)):
                        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name} cap={cap}: output {q} differs from the default cap's"
                else:
                    run_refused(G, op, f"cap={cap}")
        assert len(seen) >= 1
        assert G.L.mgk_debug_set_max_partials(G.ctx, 0) == 0
        run_ok(G, op, SLOTS, "cap restored")
    except BaseException:
        G.release()
        G.L.mgk_set_tuning(-1, -1)
        G.L.mgk_debug_set_max_partials(G.ctx, 0)
        raise
    _finish(G, P, name)


@pytest.mark.parametrize("name,shape,variants,cap_tuning,kind", _cases(kinds=False))
def test_launchers_hold_their_count_to_a_lowered_cap(mgk, orc, name, shape, variants, cap_tuning, kind):
    body_lowered_caps(mgk, orc, name, shape, cap_tuning, kind)


def test_the_cap_setter_takes_1_to_16384_and_never_raises_the_cap(mgk):
    L = mgk.L
    n = C.c_long()
    assert L.mgk_debug_partials(mgk.ctx, C.byref(n)) and n.value == 3 * SLOTS
    try:
        for bad in (-1, SLOTS + 1, 1 << 30):
            assert L.mgk_debug_set_max_partials(mgk.ctx, bad) == EINVAL
        for ok in (1, 7, SLOTS, 0):
            assert L.mgk_debug_set_max_partials(mgk.ctx, ok) == 0
        assert L.mgk_debug_set_max_partials(None, 4) == EINVAL and not L.mgk_debug_partials(None, None)
    finally:
        L.mgk_debug_set_max_partials(mgk.ctx, 0)


# ---- d. the range forms -----------------------------------------------------------------------------------------------------------
def _ranges(spec, nm):
    return [(a % nm if a < 0 else a, nm if b is None else (b % nm if b < 0 else b)) for a, b in spec]


def body_range_groups(mgk, orc, name, shape, kind, host=False):
    G, P, op = _session(mgk, orc, name, shape, kind)
    try:
        one = _range_call(P, name, op.outs[0][1])
        nm = P.nz if P.dim == 3 else P.ny
        ranges = _ranges(RANGE_FORMS[name], nm)
        assert sorted(ranges)[0][0] == 0 and sorted(ranges)[-1][1] == nm and sum(b - a for a, b in ranges) == nm
        off, parts, np_ = 0, [], C.c_int()
        for z0, z1 in ranges:
            np_.value = -1
            rc = one(z0, z1, off, np_)
            assert rc == 0, f"{name} [{z0}, {z1}) at slot {off}: rc {rc}: {G.last_error()}"
            assert np_.value >= 1
            parts.append((off, np_.value))
            off += np_.value
            wr = ~is_poison(G.read_scratch())
            assert wr[:off].all() and not wr[off:].any(), (f"{name} [{z0}, {z1}): the slot intervals {parts} are not what is written: "
                                                           f"{[int(q) for q in np.flatnonzero(wr)[:4]]} .. {[int(q) for q in np.flatnonzero(wr)[-4:]]}")
        assert G.scratch_poisoned_calls[name] == 1, "only the first range of a group may be preceded by the poison"
        s = G.read_scratch()[:off]
        assert np.all(np.isfinite(s)) and np.all(s >= 0.0)
        ss = C.c_double(-1.0)
        G._chk(G.L.mgk_partials_finish(G.ctx, off, C.byref(ss), None))
        assert _close(ss.value, op.want[0]), f"{name}: the three ranges sum to {ss.value!r}, the whole grid's norm is {op.want[0]!r}"
        assert abs(math.fsum(s) - ss.value) <= RED_RTOL * ss.value
        check_outs(op, fetch_outs(G, op), "three ranges")
        # a cap that leaves one slot less after part_off than the second range took: refit within the room, or refuse; nothing at or beyond the cap
        if not host:
            (o1, n1), (o2, n2) = parts[0], parts[1]
            z0, z1 = ranges[0]
            for cap in sorted({n1 + n2 - 1, n1 + 1, n1}):
                G._chk(one(z0, z1, 0, np_))                      # (opens a new group: the proxy poisons the scratch)
                assert np_.value == n1
                with capped(G, cap):
                    np_.value = -1
                    rc = one(ranges[1][0], ranges[1][1], n1, np_)
                    wr = ~is_poison(G.read_scratch())
                    assert not wr[cap:].any(), f"{name}: under the cap {cap} the slots {[int(q) for q in np.flatnonzero(wr[cap:])[:6] + cap]} were written"
                    if rc == 0:
                        assert 1 <= np_.value <= cap - n1 and wr[:n1 + np_.value].all() and not wr[n1 + np_.value:].any()
                    else:
                        msg = G.last_error()
                        assert rc == EINVAL and "partial" in msg, msg
                        assert wr[:n1].all() and not wr[n1:].any(), f"{name}: refused under the cap {cap}, yet slots after {n1} were written"
    except BaseException:
        G.release()
        G.L.mgk_debug_set_max_partials(G.ctx, 0)
        raise
    _finish(G, P, name)


RANGE_CASES = [pytest.param(name, shape, id=f"{name}-{_sid(shape)}") for name in RANGE_FORMS for shape, _, _ in SHAPES[name]]


@pytest.mark.parametrize("name,shape", RANGE_CASES)
def test_range_forms_fill_disjoint_slot_intervals(mgk, orc, name, shape):
    body_range_groups(mgk, orc, name, shape, "level")


# ---- e. deferred results ----------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def body_deferred(mgk, orc, name, shape, kind="level"):
    G, P, op = _session(mgk, orc, name, shape, kind)
    try:
        L = G.L
        assert op.deferrable == (name not in OWN_PROTOCOL)
        assert op.call() == 0
        sync_vals = list(op.values)
        check_values(op)
        slots = G.upload(np.full(4, SENT))
        try:
            G._chk(L.mgk_defer_result(G.ctx, C.c_void_p(slots.value + 8)))
            rc = op.call()
        finally:
            G._chk(L.mgk_defer_result(G.ctx, None))
        assert rc == 0
        G.sync()
        got = G.download(slots, 4)                               # (checks the guard zones of the four doubles)
        if op.deferrable:
            assert op.values == [0.0] and math.copysign(1.0, op.values[0]) == 1.0, f"{name}: a deferred call returned {op.values} to the host"
            assert _bits(got[1]) == _bits(sync_vals[0]), f"{name}: the deferred slot holds {got[1]!r}, the synchronous call returns {sync_vals[0]!r}"
        else:
            assert [_bits(v) for v in op.values] == [_bits(v) for v in sync_vals], f"{name}: a pending deferral changed its results"
            assert got[1] == SENT, f"{name}: wrote the caller's deferred slot"
        assert got[0] == SENT and got[2] == SENT and got[3] == SENT, f"{name}: the neighbours of the deferred slot were written: {got}"
        assert op.call() == 0
        assert [_bits(v) for v in op.values] == [_bits(v) for v in sync_vals], f"{name}: after mgk_defer_result(NULL) the synchronous value is not back"
        G.free(slots)
    except BaseException:
        G.L.mgk_defer_result(G.ctx, None)
        G.release()
        raise
    _finish(G, P, name)


DEFER_CASES = [pytest.param(name, shapes[0][0], id=f"{name}-{_sid(shapes[0][0])}") for name, shapes in SHAPES.items()]


@pytest.mark.parametrize("name,shape", DEFER_CASES)
def test_deferred_result_lands_in_the_callers_slot_alone(mgk, orc, name, shape):
    body_deferred(mgk, orc, name, shape)


def test_krylov_fetch_is_untouched_by_a_pending_deferral(mgk, orc):
    """mgk_multi_axpy_sumsq_f64 with NULL for sumsq_host + mgk_krylov_fetch: its own deferral; mgk_defer_result does not reroute it"""
    G, P, op = _session(mgk, orc, "mgk_multi_axpy_sumsq_f64", CUBE, "level")
    try:
        assert op.call() == 0
        want = op.values[0]
        slots = G.upload(np.full(4, SENT))
        ptrs, hdev = op.keep
        op.prepare()
        w2 = op.outs[0][1]
        try:
            G._chk(G.L.mgk_defer_result(G.ctx, C.c_void_p(slots.value + 8)))
            G._chk(G.L.mgk_multi_axpy_sumsq_f64(G.ctx, P.gp, KRY_K, hdev, ptrs, w2, None, None))
            ss = C.c_double(-1.0)
            G._chk(G.L.mgk_krylov_fetch(G.ctx, 0, None, C.byref(ss), None))
        finally:
            G._chk(G.L.mgk_defer_result(G.ctx, None))
        assert _bits(ss.value) == _bits(want)
        assert np.all(G.download(slots, 4) == SENT)
        G.free(slots)
    except BaseException:
        G.L.mgk_defer_result(G.ctx, None)
        G.release()
        raise
    _finish(G, P, "mgk_multi_axpy_sumsq_f64")


# ---- f. two solves ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,npts,levels", [(2, 129, 6), (3, 33, 4)])
def test_a_solve_does_not_read_what_the_scratch_held(mgk, dim, npts, levels):
    """the product's own sequence: norms of differently sized levels alternating on one scratch.  Poisoned before solve(), the solve returns
    the same iteration count, residual history and solution bit for bit"""
    from multigrid_petsc_amd.solver import Solver
    L = mgk.L
    runs = []
    for poison in (False, True):
        s = Solver(dim, npts, levels, v=(3, 3), maxiter=50, scale=6.0 / 7.0)
        try:
            s.set_rhs_problem()
            if poison:
                ctx, n = s.kernel_ctx, C.c_long()
                p = L.mgk_debug_partials(ctx, C.byref(n))
                assert p and n.value == 3 * SLOTS
                fill = np.full(n.value, np.array([0x7FF80000DEADBEEF], dtype=np.uint64).view(np.float64)[0])
                s.sync()
                assert L.mgk_h2d(ctx, C.c_void_p(p), fill.ctypes.data_as(C.c_void_p), fill.nbytes) == 0
            it = s.solve()
            runs.append((it, s.rnorm.copy(), s.solution()))
        finally:
            s.close()
    (it0, r0, u0), (it1, r1, u1) = runs
    assert 1 <= it0 < 50 and it1 == it0
    assert np.all(np.isfinite(r1)) and np.array_equal(r0.view(np.uint64), r1.view(np.uint64)), f"residual histories differ: {r0} vs {r1}"
    assert np.array_equal(u0.view(np.uint64), u1.view(np.uint64))


def test_every_reducer_has_a_case_a_verdict_and_a_deferral_row():
    assert set(BUILDERS) == set(REDUCERS) == set(SHAPES)
    assert set(OWN_PROTOCOL) <= set(REDUCERS) and set(RANGE_FORMS) == {n for n, off in REDUCERS.items() if off is not None}
