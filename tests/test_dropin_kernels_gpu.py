"""GPU parity of the kernels behind the PETSc-surface drop-in (csrc/petsc_shim.c) that only whole-program tests reached before: the flat
BLAS-1 kernels, the generic AIJ SpMV, the dense coarse solve, the I-cycle's level operator, the stretched-mesh (row-table) forms and the
LDS tails PCMG records.  Each entry point is called directly through the C ABI (include/mgk.h) and compared with a plain float64 numpy
statement of its contract, or with the oracle -- never with another GPU run.

Exact where the contract fixes the arithmetic: the build uses -ffp-contract=off, so numpy's separately rounded products and sums in the
same parenthesisation give the same bits.  mgk_flat_dot and mgk_dense_mult_f64 do not fix their summation order; they are held to a
forward-error bound derived from the reduction the kernel runs, and to bitwise reproducibility.

flat_grid() launches at most 8192 blocks of 256 lanes (CAP = 2^21 elements or rows per pass): every size above CAP runs a second
grid-stride pass of the flat kernels, of k_flat_dot and of k_csr_mult (whose waves then re-stage their LDS window)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from oracle import Oracle
from row_tables import _rt_apply, _rt_jacobi, _rt_tables

pytestmark = pytest.mark.gpu
CAP = 8192 * 256                 # elements / rows covered by one grid-stride pass of flat_grid()'s launch
TAIL = 64                        # sentinel doubles allocated past n
U = 2.0 ** -53


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _gamma(k):
    return k * U / (1.0 - k * U)


def _upload_raw(mgk, arr, dtype):
    arr = np.ascontiguousarray(arr, dtype=dtype)
    p = mgk.alloc(max(arr.nbytes, 8))
    if arr.nbytes:
        mgk._chk(mgk.L.mgk_h2d(mgk.ctx, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes))
    return p


def _sentinel(m):
    return 1000.0 + 0.125 * np.arange(m)


def _padded(g, interior, fill):
    """whole padded allocation of a 2-D geometry: `interior` (n x n) at its place, `fill` everywhere else (ghosts, padding)"""
    raw = np.full(g.total, fill, dtype=np.float64)
    raw[_interior_index(g)] = np.asarray(interior, dtype=np.float64).ravel()
    return raw


def _interior_index(g):
    i, j = np.divmod(np.arange(g.nx * g.ny), g.nx)
    return g.org + i * g.pitch + j


# ------------------------------------------------------------------------------------------------------------------------------
# flat BLAS-1 kernels
# ------------------------------------------------------------------------------------------------------------------------------
FLAT_SIZES = [1, 63, 64, 255, 256, 257, CAP - 1, CAP, CAP + 1, 3 * CAP + 12345, "geom2d_4095"]
SCALARS = (0.0, -0.0, 1.0, -2.5)
# zeros, subnormals (smallest, largest, and values whose products underflow to subnormals), infinities, NaN, overflow
SPECIALS = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -1.5e-310, 1e-160, -3e-155, np.inf, -np.inf, np.nan,
                     1.0, -2.5, 1.7e308, -0.75])
K3 = SPECIALS.size ** 3


def _flat_n(mgk, n):
    return mgk.geom(2, 4095).total if n == "geom2d_4095" else n


def _flat_inputs(n, seed):
    """x, y, z of n values (+ TAIL sentinels): normal random values with a quarter of them scaled to extreme magnitudes, and every triple of
    SPECIALS in the first half (and at the end of large arrays, in the last grid-stride pass)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        v = rng.standard_normal(n)          # full 53-bit significands (uniform(-1, 1) draws sit on a 2^-52 grid: their sums are exact)
        wide = rng.random(n) < 0.25
        v[wide] *= 10.0 ** rng.integers(-320, 306, int(wide.sum())).astype(np.float64)
        out.append(v)
    k = SPECIALS.size
    t = np.arange(K3)
    trip = (SPECIALS[t % k], SPECIALS[(t // k) % k], SPECIALS[t // (k * k)])
    for start in ([0] + ([n - K3] if n >= 4 * K3 else [])):
        m = min(K3, n // 2)                 # at least half of every array stays random
        for v, s in zip(out, trip):
            v[start:start + m] = s[:m]
    return [np.concatenate([v, _sentinel(TAIL)]) for v in out]


def _scalar_sets(n, nscal):
    """every combination on small arrays; on large ones four sets that put every value in every position, and every set of
    nonzero values (a zero coefficient would hide the order of the remaining terms)"""
    if nscal == 0:
        return [()]
    if n <= 257:
        return list(itertools.product(SCALARS, repeat=nscal))
    rot = [tuple(SCALARS[(q + p) % 4] for p in range(nscal)) for q in range(4)]
    return rot + [sc for sc in itertools.product((1.0, -2.5), repeat=nscal) if sc not in rot]


def _assert_flat(got, want, n, what):
    g, w = got[:n], want[:n]
    wn = np.isnan(w)
    assert np.isnan(g[wn]).all(), f"{what}: numpy gives NaN where the kernel does not"
    bad = (_bits(g) != _bits(w)) & ~wn
    if bad.any():
        q = np.flatnonzero(bad)[:6]
        pytest.fail(f"{what}: {int(bad.sum())} of {n} results differ; first at {q.tolist()}: got {g[q].tolist()} want {w[q].tolist()}")
    assert np.array_equal(_bits(got[n:]), _bits(_sentinel(TAIL))), f"{what}: wrote past n"


@pytest.mark.parametrize("n", FLAT_SIZES)
def test_flat_kernels_bit_exact(mgk, n):
    """VecAXPY / VecAYPX / VecAXPBYPCZ / VecSet / VecScale / VecPointwiseMult as mgk_flat_*: every element equals numpy's evaluation of
    the kernel's expression bit for bit (NaN only where numpy gives NaN), the TAIL doubles past n are never written"""
    n = _flat_n(mgk, n)
    x, y, z = _flat_inputs(n, 31 + n % 1000)
    m = n + TAIL
    dx, dy, dz0, dz = _upload_raw(mgk, x, np.float64), _upload_raw(mgk, y, np.float64), _upload_raw(mgk, z, np.float64), mgk.alloc(8 * m)
    L, ctx = mgk.L, mgk.ctx
    X, Y, Z = x[:n], y[:n], z[:n]
    ops = {
        "axpy": (1, lambda a: Z + a * X, lambda a: L.mgk_flat_axpy(ctx, n, a, dx, dz, None)),
        "aypx": (1, lambda a: X + a * Z, lambda a: L.mgk_flat_aypx(ctx, n, a, dx, dz, None)),
        "axpbypcz": (3, lambda a, b, c: (a * X + b * Y) + c * Z, lambda a, b, c: L.mgk_flat_axpbypcz(ctx, n, a, b, c, dx, dy, dz, None)),
        "fill": (1, lambda a: np.full(n, a), lambda a: L.mgk_flat_fill(ctx, n, a, dz, None)),
        "scale": (1, lambda a: a * Z, lambda a: L.mgk_flat_scale(ctx, n, a, dz, None)),
        "pointwise_mult": (0, lambda: X * Y, lambda: L.mgk_flat_pointwise_mult(ctx, n, dx, dy, dz, None)),
    }
    try:
        with np.errstate(all="ignore"):
            for name, (nscal, ref, run) in ops.items():
                for sc in _scalar_sets(n, nscal):
                    mgk._chk(L.mgk_d2d(ctx, dz, dz0, 8 * m, None))
                    mgk._chk(run(*sc))
                    mgk.sync()
                    _assert_flat(mgk.download(dz, m), ref(*sc), n, f"{name}{sc} n={n}")
        # the inputs are read only
        assert np.array_equal(_bits(mgk.download(dx, m)), _bits(x)) and np.array_equal(_bits(mgk.download(dy, m)), _bits(y))
    finally:
        for p in (dx, dy, dz0, dz):
            mgk.free(p)


# ------------------------------------------------------------------------------------------------------------------------------
# mgk_flat_dot
# ------------------------------------------------------------------------------------------------------------------------------
def _dot_depth(n):
    """Longest chain of roundings from a product to the result in k_flat_dot + k_finish_sum (mgk_kernels.hip):
       G = flat_grid(n) = min(ceil(n / 256), 8192) blocks (below the context's 16384 partial slots);
       - each lane: one sequential chain acc = 0 + p + p + ... over ceil(n / (256 G)) products;
       - wave_sum: 6 shuffle-tree steps;  block_sum: thread 0 adds the 4 wave sums in sequence (4 additions);
       - k_finish_sum over the G partials: one chain of ceil(G / 256) per lane, 6 tree steps, 4 wave sums in sequence.
    Every result is a sum over a tree of depth K = ceil(n / (256 G)) + 6 + 4 + ceil(G / 256) + 6 + 4, so that
    |got - sum p| <= gamma_K sum |p| (Higham, Accuracy and Stability, eq. 4.4), gamma_K = K u / (1 - K u)."""
    G = max(1, min((n + 255) // 256, 8192))
    return -(-n // (256 * G)) + 6 + 4 + -(-G // 256) + 6 + 4


def _dot_inputs(n, seed, cancel):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-6, 7, n).astype(np.float64)
    y = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-6, 7, n).astype(np.float64)
    if cancel:                          # products in +p / -p pairs: sum p = 0 exactly, sum |p| large
        h = n // 2
        x[h:2 * h], y[h:2 * h] = x[:h], -y[:h]
        if n % 2:
            x[-1] = 0.0
    return x, y


@pytest.mark.parametrize("n", FLAT_SIZES)
def test_flat_dot_error_bound_reproducibility_and_deferred_slot(mgk, n):
    """VecDot / VecNorm^2: (1) within gamma_K sum|p| of the exactly rounded sum of the rounded products (math.fsum), K from
    _dot_depth; (2) bit-identical across calls; (3) with a deferred slot set (mgk_defer_result) the host gets 0.0 and the slot the
    immediate result's bits.  Random products, and a cancelling set whose exact sum is 0."""
    n = _flat_n(mgk, n)
    K = _dot_depth(n)
    L = mgk.L
    slot = mgk.alloc(8)
    for cancel in ((False, True) if n >= 2 else (False,)):
        x, y = _dot_inputs(n, 77 + n % 1000 + cancel, cancel)
        dx, dy = mgk.upload(x), mgk.upload(y)
        p = x * y
        exact, mag = math.fsum(p), math.fsum(np.abs(p))
        got, again = C.c_double(), C.c_double()
        mgk._chk(L.mgk_flat_dot(mgk.ctx, n, dx, dy, C.byref(got), None))
        assert abs(got.value - exact) <= _gamma(K) * mag * (1 + 4 * U), f"n={n} cancel={cancel}: {got.value} vs {exact}, K={K}"
        if cancel:
            assert exact == 0.0 and mag > 0
        mgk._chk(L.mgk_flat_dot(mgk.ctx, n, dx, dy, C.byref(again), None))
        assert _bits(got.value) == _bits(again.value)
        host = C.c_double(-1.0)
        mgk._chk(L.mgk_memset0(mgk.ctx, slot, 8, None))
        try:
            mgk._chk(L.mgk_defer_result(mgk.ctx, slot))
            mgk._chk(L.mgk_flat_dot(mgk.ctx, n, dx, dy, C.byref(host), None))
        finally:
            mgk._chk(L.mgk_defer_result(mgk.ctx, None))
        mgk.sync()
        assert host.value == 0.0
        assert _bits(mgk.download(slot, 1)[0]) == _bits(got.value)
        # reset: the immediate form delivers again
        mgk._chk(L.mgk_flat_dot(mgk.ctx, n, dx, dy, C.byref(host), None))
        assert _bits(host.value) == _bits(got.value)
        mgk.free(dx)
        mgk.free(dy)
    mgk.free(slot)


# ------------------------------------------------------------------------------------------------------------------------------
# mgk_csr_mult_f64
# ------------------------------------------------------------------------------------------------------------------------------
def _csr_ref(rowptr, col, val, x):
    """one running sum per row, 0.0 + v0 x[c0] + v1 x[c1] + ... in stored order, each product rounded first"""
    nrows = rowptr.size - 1
    lens = np.diff(rowptr)
    s = np.zeros(nrows)
    order = np.argsort(-lens, kind="stable")
    neg = -lens[order]
    for k in range(int(lens.max()) if nrows else 0):
        r = order[:np.searchsorted(neg, -k, side="left")]          # rows with more than k entries
        q = rowptr[r] + k
        s[r] = s[r] + val[q] * x[col[q]]
    return s


def _csr_build(rng, lens, nx):
    """ascending, distinct columns per row (random gaps), random values"""
    lens = np.asarray(lens, dtype=np.int64)
    nrows = lens.size
    rowptr = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    nnz = int(rowptr[-1])
    gaps = rng.integers(1, 50, nnz)
    cs = np.cumsum(gaps)
    row_of = np.repeat(np.arange(nrows), lens)
    within = cs - cs[rowptr[:-1][row_of]]
    start = rng.integers(0, nx - 49 * lens)
    col = (start[row_of] + within).astype(np.int32)
    assert nnz == 0 or (col.min() >= 0 and col.max() < nx)
    return rowptr, col, rng.uniform(-2.0, 2.0, nnz)


WAVES = 8192 * 4                 # waves of k_csr_mult's largest launch; wave w owns the 64-row groups w, w + WAVES, ...


def _csr_lengths(rng, nrows, long_rows):
    """5/9/14-entry rows (the reference's operators), one-entry and empty rows; with long_rows, the first 16 waves and every
    1021st one alternate between groups staged in LDS and groups of more than CSR_CAP = 1024 entries (one row of 1100) from one
    grid-stride pass to the next"""
    lens = rng.choice(np.array([0, 1, 5, 9, 14]), size=nrows, p=[0.1, 0.2, 0.4, 0.2, 0.1])
    if long_rows:
        for g in range((nrows + 63) // 64):
            w = g % WAVES
            if (w < 16 or w % 1021 == 0) and (g // WAVES + w) % 2 == 0:
                lens[64 * g] = 1100
    return lens


def _csr_run(mgk, rowptr, col, val, x, nrows, y0, alpha, addto, mode, row_map=(0, 0, 0)):
    """mode: 'none' (addto = NULL), 'other' (addto != y), 'same' (addto == y).  y0 / addto: whole device arrays as numpy"""
    L = mgk.L
    drp, dcol, dval, dx = _upload_raw(mgk, rowptr, np.int64), _upload_raw(mgk, col, np.int32), mgk.upload(val) if val.size else mgk.alloc(8), mgk.upload(x)
    dy = mgk.upload(y0)
    dadd = dy if mode == "same" else (mgk.upload(addto) if mode == "other" else None)
    try:
        mgk._chk(L.mgk_csr_mult_f64(mgk.ctx, nrows, drp, dcol, dval, dx, dy, alpha, dadd, row_map[0], row_map[1], row_map[2], None))
        mgk.sync()
        return mgk.download(dy, y0.size)
    finally:
        for p in (drp, dcol, dval, dx, dy) + ((dadd,) if mode == "other" else ()):
            mgk.free(p)


def _csr_expect(s, y0, alpha, addto, mode, rows_at):
    want = y0.copy()
    base = {"none": None, "other": addto, "same": y0}[mode]
    want[rows_at] = s if base is None else base[rows_at] + alpha * s
    return want


CSR_MODES = (("none", 1.0), ("other", -0.7), ("same", 2.5))


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, CAP - 1, CAP + 1, 2 * CAP + 100])
@pytest.mark.parametrize("long_rows", [False, True])
def test_csr_mult_bit_exact(mgk, nrows, long_rows):
    """generic AIJ SpMV: y = A x, y = addto + alpha (A x) into another array and in place (the shim passes addto == y): exact against
    numpy's sequential row sums; nothing past nrows is written.  2 CAP + 100 rows: waves 0 and 1 make three grid-stride passes and
    re-stage their LDS window, with long_rows alternating staged / unstaged groups between passes"""
    rng = np.random.default_rng(5100 + nrows + long_rows)
    nx = nrows + 60000
    rowptr, col, val = _csr_build(rng, _csr_lengths(rng, nrows, long_rows), nx)
    x = rng.uniform(-1.0, 1.0, nx)
    s = _csr_ref(rowptr, col, val, x)
    rows_at = np.arange(nrows)
    for mode, alpha in CSR_MODES:
        y0 = np.concatenate([rng.uniform(-1.0, 1.0, nrows), _sentinel(TAIL)])
        addto = np.concatenate([rng.uniform(-1.0, 1.0, nrows), _sentinel(TAIL)]) if mode == "other" else None
        got = _csr_run(mgk, rowptr, col, val, x, nrows, y0, alpha, addto, mode)
        want = _csr_expect(s, y0, alpha, addto, mode, rows_at)
        bad = _bits(got) != _bits(want)
        assert not bad.any(), f"{mode}: {int(bad.sum())} rows differ, first {np.flatnonzero(bad)[:5].tolist()}"


def test_csr_mult_group_sizes_at_the_staging_cap(mgk):
    """64-row groups of exactly CSR_CAP = 1024 entries (staged) and of 1025 (read from global memory), spread over the rows of the
    group or held by one row, next to a group of two 600-entry rows and one of short rows"""
    rng = np.random.default_rng(5200)
    groups = [np.full(64, 16), np.r_[np.full(63, 16), 17], np.r_[1024, np.zeros(63, int)], np.r_[1025, np.zeros(63, int)],
              np.r_[600, 600, np.zeros(62, int)], rng.choice([0, 1, 5, 9, 14], 64), np.r_[np.zeros(63, int), 1025], np.full(64, 16)]
    lens = np.concatenate(groups)
    assert [int(g.sum()) for g in groups[:4]] == [1024, 1025, 1024, 1025]
    nrows, nx = lens.size, 200000
    rowptr, col, val = _csr_build(rng, lens, nx)
    x = rng.uniform(-1.0, 1.0, nx)
    s = _csr_ref(rowptr, col, val, x)
    for mode, alpha in CSR_MODES:
        y0 = np.concatenate([rng.uniform(-1.0, 1.0, nrows), _sentinel(TAIL)])
        addto = np.concatenate([rng.uniform(-1.0, 1.0, nrows), _sentinel(TAIL)]) if mode == "other" else None
        got = _csr_run(mgk, rowptr, col, val, x, nrows, y0, alpha, addto, mode)
        want = _csr_expect(s, y0, alpha, addto, mode, np.arange(nrows))
        assert np.array_equal(_bits(got), _bits(want)), f"{mode}: rows {np.flatnonzero(_bits(got) != _bits(want))[:8].tolist()}"


@pytest.mark.parametrize("n", [63, 2047])
def test_csr_mult_into_a_padded_grid_field(mgk, n):
    """row_n / row_pitch / row_org: row r lands at org + (r / n) pitch + r % n of a padded 2-D field; a 5-point operator whose columns
    are offsets into a padded x.  Ghosts and padding of y (sentinels) stay untouched.  2047^2 rows: a second grid-stride pass."""
    rng = np.random.default_rng(5300 + n)
    g = mgk.geom(2, n)
    at = _interior_index(g)
    nrows = n * n
    offs = np.array([-g.pitch, -1, 0, 1, g.pitch])
    rowptr = np.arange(0, 5 * nrows + 1, 5, dtype=np.int64)
    col = (at[:, None] + offs[None, :]).ravel().astype(np.int32)
    val = rng.uniform(-2.0, 2.0, 5 * nrows)
    x = _padded(g, rng.uniform(-1.0, 1.0, nrows), 0.0)
    s = _csr_ref(rowptr, col, val, x)
    for mode, alpha in CSR_MODES:
        y0 = _padded(g, rng.uniform(-1.0, 1.0, nrows), 0.0)
        y0[np.setdiff1d(np.arange(g.total), at)] = _sentinel(g.total - nrows)
        addto = _padded(g, rng.uniform(-1.0, 1.0, nrows), -7.0) if mode == "other" else None
        got = _csr_run(mgk, rowptr, col, val, x, nrows, y0, alpha, addto, mode, (n, g.pitch, g.org))
        want = _csr_expect(s, y0, alpha, addto, mode, at)
        assert np.array_equal(_bits(got), _bits(want)), f"{mode}: {int((_bits(got) != _bits(want)).sum())} differ"


@pytest.mark.parametrize("which,dim,npts", [("A", 2, 65), ("R", 2, 65), ("P", 2, 65), ("A", 3, 17)])
def test_csr_mult_on_the_oracle_operators(mgk, orc, which, dim, npts):
    """the reference's assembled operators (the oracle's CSR leg): MatMult through the generic kernel == the oracle's csr_mult"""
    m = orc.build(which, dim, npts, 0)
    rows = orc.csr_rows(m)
    nrows, ncols = orc.L.mgo_csr_nrows(m), orc.L.mgo_csr_ncols(m)
    rowptr = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum([c.size for c, _ in rows], out=rowptr[1:])
    col = np.concatenate([c for c, _ in rows]).astype(np.int32)
    val = np.concatenate([v for _, v in rows])
    x = np.random.default_rng(5400).uniform(-1.0, 1.0, ncols)
    want = orc.csr_mult(m, x)
    orc.L.mgo_csr_free(m)
    got = _csr_run(mgk, rowptr, col, val, x, nrows, np.zeros(nrows), 1.0, None, "none")
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(want), _bits(_csr_ref(rowptr, col, val, x)))


# ------------------------------------------------------------------------------------------------------------------------------
# mgk_dense_mult_f64 (PCMG's exact coarse solve)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 4, 5, 63, 1023])
def test_dense_mult_error_bound_and_reproducibility(mgk, m):
    """y = B x, one wave per row: each lane sums ceil(n / 64) products in sequence from 0, then a 6-step shuffle tree, so
    |y_i - sum_j p_ij| <= gamma_K sum_j |p_ij| with K = ceil(n / 64) + 6 against math.fsum of the rounded products; two calls give
    the same bits; nothing past m is written"""
    rng = np.random.default_rng(5500 + m)
    for n in (1, 63, 64, 65, 1000):
        B = rng.uniform(-1.0, 1.0, (m, n)) * 10.0 ** rng.integers(-4, 5, (m, n)).astype(np.float64)
        x = rng.uniform(-1.0, 1.0, n)
        dB, dx, dy = mgk.upload(B.ravel()), mgk.upload(x), mgk.upload(np.concatenate([np.zeros(m), _sentinel(TAIL)]))
        mgk._chk(mgk.L.mgk_dense_mult_f64(mgk.ctx, m, n, dB, dx, dy, None))
        mgk.sync()
        got = mgk.download(dy, m + TAIL)
        mgk._chk(mgk.L.mgk_dense_mult_f64(mgk.ctx, m, n, dB, dx, dy, None))
        mgk.sync()
        again = mgk.download(dy, m + TAIL)
        P = B * x[None, :]
        K = -(-n // 64) + 6
        for i in range(m):
            exact, mag = math.fsum(P[i]), math.fsum(np.abs(P[i]))
            assert abs(got[i] - exact) <= _gamma(K) * mag * (1 + 4 * U), f"m={m} n={n} row {i}: {got[i]} vs {exact}"
        assert np.array_equal(_bits(got), _bits(again))
        assert np.array_equal(_bits(got[m:]), _bits(_sentinel(TAIL)))
        for p in (dB, dx, dy):
            mgk.free(p)


# ------------------------------------------------------------------------------------------------------------------------------
# the I-cycle's level operator of several grids: mgk_apply_add_f64, mgk_window_add_f64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 7, 63, 255, 2047, 2049, 4095])
def test_apply_add_bit_exact(mgk, n):
    """y += A x, z = y; z = z + c0 x(i-1,j); + c1 x(i,j-1); + c2 x(i,j); + c3 x(i,j+1); + c4 x(i+1,j): exact; 4095 rows cross the
    2048-row cap of grid.y; y's ghosts and padding (sentinels) unchanged"""
    rng = np.random.default_rng(5600 + n)
    g = mgk.geom(2, n)
    c = rng.uniform(-3.0, 3.0, 5)
    X = rng.uniform(-1.0, 1.0, (n, n))
    Y = rng.uniform(-1.0, 1.0, (n, n))
    xr = _padded(g, X, 0.0)
    yr = _padded(g, Y, 0.0)
    at = _interior_index(g)
    yr[np.setdiff1d(np.arange(g.total), at)] = _sentinel(g.total - n * n)
    p = np.zeros((n + 2, n + 2))
    p[1:-1, 1:-1] = X
    z = Y.copy()
    z = z + c[0] * p[:-2, 1:-1]
    z = z + c[1] * p[1:-1, :-2]
    z = z + c[2] * p[1:-1, 1:-1]
    z = z + c[3] * p[1:-1, 2:]
    z = z + c[4] * p[2:, 1:-1]
    want = yr.copy()
    want[at] = z.ravel()
    dx, dy = mgk.upload(xr), mgk.upload(yr)
    mgk._chk(mgk.L.mgk_apply_add_f64(mgk.ctx, C.byref(g), mgk.coef(list(c)), dx, dy, None))
    mgk.sync()
    got = mgk.download(dy, g.total)
    assert np.array_equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} differ"
    assert np.array_equal(mgk.download(dx, g.total), xr)
    mgk.free(dx)
    mgk.free(dy)


def _window_ref(Y, wt, XC, S):
    """yf(i,j) += w[i - S ic][j - S jc] xc(ic,jc) over the coarse points with S ic <= i <= S ic + 2S - 2 (same for j), ascending
    coarse index (ic major)"""
    nf, nc = Y.shape[0], XC.shape[0]
    W = 2 * S - 1
    idx = np.arange(nf)
    one = (idx + 1) % S == 0
    c0 = idx // S - np.where(one, 0, 1)             # first parent (may be -1: outside the grid)
    y = Y.copy()
    for pi in (0, 1):
        ic = c0 + pi
        vi = (pi < np.where(one, 1, 2)) & (ic >= 0) & (ic < nc)
        for qj in (0, 1):
            jc = c0 + qj
            vj = (qj < np.where(one, 1, 2)) & (jc >= 0) & (jc < nc)
            m = vi[:, None] & vj[None, :]
            di = (idx - S * ic)[:, None]
            dj = (idx - S * jc)[None, :]
            wv = wt[np.clip(di, 0, W - 1), np.clip(dj, 0, W - 1)]
            xv = XC[np.clip(ic, 0, nc - 1)[:, None], np.clip(jc, 0, nc - 1)[None, :]]
            y = np.where(m, y + wv * xv, y)
    return y


@pytest.mark.parametrize("S,nc", [(2, 1), (2, 3), (2, 5), (2, 2047), (4, 1), (4, 3), (4, 5), (4, 15), (8, 1), (8, 3), (8, 7), (16, 1), (16, 3)])
def test_window_add_bit_exact(mgk, S, nc):
    """the upper blocks of the level operator: exact against numpy in ascending coarse index; nf = S (nc + 1) - 1 (nc = 1: the
    smallest window grid; S = 2, nc = 2047: nf = 4095 crosses the 2048-row cap of grid.y); xc with a zero ghost ring; yf's ghosts
    and padding (sentinels) unchanged"""
    nf = S * (nc + 1) - 1
    rng = np.random.default_rng(5700 + 31 * S + nc)
    gf, gc = mgk.geom(2, nf), mgk.geom(2, nc)
    wt = rng.uniform(-1.0, 1.0, (2 * S - 1, 2 * S - 1))
    XC = rng.uniform(-1.0, 1.0, (nc, nc))
    Y = rng.uniform(-1.0, 1.0, (nf, nf))
    yr = _padded(gf, Y, 0.0)
    at = _interior_index(gf)
    yr[np.setdiff1d(np.arange(gf.total), at)] = _sentinel(gf.total - nf * nf)
    want = yr.copy()
    want[at] = _window_ref(Y, wt, XC, S).ravel()
    dw, dxc, dy = mgk.upload(wt.ravel()), mgk.upload(_padded(gc, XC, 0.0)), mgk.upload(yr)
    mgk._chk(mgk.L.mgk_window_add_f64(mgk.ctx, C.byref(gf), C.byref(gc), S, dw, dxc, dy, None))
    mgk.sync()
    got = mgk.download(dy, gf.total)
    assert np.array_equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} differ"
    for p in (dw, dxc, dy):
        mgk.free(p)


# ------------------------------------------------------------------------------------------------------------------------------
# stretched meshes: the row-table forms
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 7, 63, 243, 255, 1023, 2047])
def test_row_table_zero_guess_two_sweep_norm_and_sweep_restrict(mgk, orc, n):
    """mgk_jacobi_zero_rowcoef_f64 (unew = scale (b dtab[i])), mgk_jacobi2_2d_sumsq_rowcoef_f64 (two sweeps + ||b - A u||^2 of the
    input) and mgk_sweep_residual_restrict_2d_rowcoef_f64 (sweep, residual of its output, full weighting, with and without the
    coarse zero-guess sweep uc0 = scale_c (bc dtab_c[ic])) against the per-operation row-table sequence: fields exact, norms 1e-12"""
    rng = np.random.default_rng(5800 + n)
    nc = (n - 1) // 2
    ct, dt = _rt_tables(rng, n)
    ctc, dtc = _rt_tables(rng, nc)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    g, gc = mgk.geom(2, n), mgk.geom(2, nc)
    L = mgk.L
    du, db, dout, dbc, duc0 = mgk.to_field(g, u.ravel()), mgk.to_field(g, b.ravel()), mgk.field(g), mgk.field(gc), mgk.field(gc)
    dct, ddt, ddtc = mgk.upload(ct.ravel()), mgk.upload(dt), mgk.upload(dtc)
    # zero-guess sweep: the whole allocation (interior + zero ghosts) is what numpy says
    mgk._chk(L.mgk_jacobi_zero_rowcoef_f64(mgk.ctx, C.byref(g), ddt, 0.8, db, dout, None))
    mgk.sync()
    assert np.array_equal(_bits(mgk.raw_field(g, dout)), _bits(_padded(g, 0.8 * (b * dt[:, None]), 0.0)))
    w1 = _rt_jacobi(ct, b, u, 0.8)
    w2 = _rt_jacobi(ct, b, w1, 0.8)
    res = b - _rt_apply(ct, u)
    nref = math.fsum((res * res).ravel())
    bc = orc.restrict(2, n, (b - _rt_apply(ct, w1)).ravel()).reshape(nc, nc)
    ss = C.c_double(0.0)
    try:
        for zc in (-1, 1, 5, 64):
            L.mgk_set_tuning(-1, zc)
            mgk._chk(L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
            mgk._chk(L.mgk_jacobi2_2d_sumsq_rowcoef_f64(mgk.ctx, C.byref(g), dct, ddt, 0.8, db, du, dout, C.byref(ss), None))
            assert np.array_equal(_bits(mgk.raw_field(g, dout)), _bits(_padded(g, w2, 0.0))), f"zc={zc}: two sweeps"
            assert abs(ss.value - nref) <= 1e-12 * nref, f"zc={zc}: norm"
            for with_uc0 in (False, True):
                for f, gg in ((dout, g), (dbc, gc), (duc0, gc)):
                    mgk._chk(L.mgk_memset0(mgk.ctx, f, 8 * gg.total, None))
                mgk._chk(L.mgk_sweep_residual_restrict_2d_rowcoef_f64(mgk.ctx, C.byref(g), C.byref(gc), dct, ddt, 0.8, db, du, dout, dbc,
                                                                      duc0 if with_uc0 else None, ddtc if with_uc0 else None, 0.6, None))
                assert np.array_equal(_bits(mgk.raw_field(g, dout)), _bits(_padded(g, w1, 0.0))), f"zc={zc} uc0={with_uc0}: swept field"
                assert np.array_equal(_bits(mgk.raw_field(gc, dbc)), _bits(_padded(gc, bc, 0.0))), f"zc={zc} uc0={with_uc0}: coarse rhs"
                want_uc0 = 0.6 * (bc * dtc[:, None]) if with_uc0 else np.zeros((nc, nc))
                assert np.array_equal(_bits(mgk.raw_field(gc, duc0)), _bits(_padded(gc, want_uc0, 0.0))), f"zc={zc} uc0={with_uc0}"
    finally:
        L.mgk_set_tuning(-1, -1)
    assert np.array_equal(mgk.from_field(g, du), u.ravel()) and np.array_equal(mgk.from_field(g, db), b.ravel())
    for p in (du, db, dout, dbc, duc0, dct, ddt, ddtc):
        mgk.free(p)


# ------------------------------------------------------------------------------------------------------------------------------
# the LDS tails: mgk_tail_cycle_cs_f64 (PCMG's recorded tail, 2-D) and mgk_tail_cycle_f32 (3-D)
# ------------------------------------------------------------------------------------------------------------------------------
def _tail_ref(ns, b0, sweep, zero_sweep, residual, restrict, prolong_add, v0, v1):
    """the tail's V-cycle stepped one operation at a time: v0 sweeps from a zero guess on every level but the last (v1 there), residual +
    full weighting down, prolongation + v0 sweeps up"""
    nlev = len(ns)

    def smooth(l, b, u, sweeps, zero):
        for it in range(sweeps):
            u = zero_sweep(l, b) if (it == 0 and zero) else sweep(l, b, u)
        return u
    B, Us = [b0], []
    for l in range(nlev):
        Us.append(smooth(l, B[l], np.zeros_like(B[l]), v1 if l == nlev - 1 else v0, True))
        if l < nlev - 1:
            B.append(restrict(l, residual(l, B[l], Us[l])))
    for l in range(nlev - 2, -1, -1):
        Us[l] = smooth(l, B[l], prolong_add(l, Us[l + 1], Us[l]), v0, False)
    return Us[0]


TAIL_CS_CASES = [(63, 6, 3, 1, 0.8, 1.0), (31, 5, 2, 1, 0.8, 1.0), (15, 4, 3, 1, 0.8, 1.0), (3, 2, 3, 1, 0.8, 1.0), (1, 1, 2, 1, 0.8, 1.0),
                 (63, 5, 3, 3, 0.8, 0.5), (15, 3, 1, 4, 0.7, 0.6), (7, 2, 0, 2, 0.9, 1.0), (31, 3, 2, 2, 0.8, 0.8), (7, 3, 4, 3, 1.0, 0.75)]


@pytest.mark.parametrize("n0,nlev,v0,v1,scale,cscale", TAIL_CS_CASES)
@pytest.mark.parametrize("form", ["coef7", "rowtab"])
def test_tail_cycle_with_coarse_scale_bit_exact(mgk, orc, n0, nlev, v0, v1, scale, cscale, form):
    """mgk_tail_cycle_cs_f64, both forms (coef7 + dinv: constant five-point coefficients in the first 5 of 7 doubles per level; ctab +
    dtab: row tables), against numpy stepping with coarse_scale on the coarsest level only -- including the 1 x 1 coarsest grid with
    v1 = 1, coarse_scale = 1 (PCMG's exact coarse solve)"""
    rng = np.random.default_rng(5900 + 7 * n0 + nlev + v0 + v1)
    ns = [n0]
    for _ in range(nlev - 1):
        ns.append((ns[-1] - 1) // 2)
    assert ns[-1] >= 1
    if form == "rowtab":
        tabs = [_rt_tables(rng, n) for n in ns]
    else:
        tabs = []
        for n in ns:
            As = rng.uniform(0.5, 1.5, 5) * (n + 1) ** 2
            As[2] = -(As[0] + As[1] + As[3] + As[4]) * rng.uniform(1.0, 1.2)
            tabs.append((np.tile(As, (n, 1)), np.full(n, 1.0 / As[2])))
    b0 = rng.uniform(-1.0, 1.0, (n0, n0))

    def sc(l):
        return cscale if l == nlev - 1 else scale

    def sweep(l, b, u):
        ct, dt = tabs[l]
        return u + sc(l) * ((b - _rt_apply(ct, u)) * dt[:, None])
    want = _tail_ref(ns, b0, sweep, lambda l, b: sc(l) * (b * tabs[l][1][:, None]), lambda l, b, u: b - _rt_apply(tabs[l][0], u),
                     lambda l, r: orc.restrict(2, ns[l], r.ravel()).reshape(ns[l + 1], ns[l + 1]),
                     lambda l, uc, uf: orc.prolong_add(2, ns[l], uc.ravel(), uf.ravel()).reshape(ns[l], ns[l]), v0, v1)
    g = mgk.geom(2, n0)
    db, du = mgk.to_field(g, b0.ravel()), mgk.field(g)
    nn = (C.c_int * nlev)(*ns)
    bufs = []
    if form == "rowtab":
        bufs = [x for ct, dt in tabs for x in (mgk.upload(ct.ravel()), mgk.upload(dt))]
        cta = (C.c_void_p * nlev)(*[bufs[2 * l].value for l in range(nlev)])
        dta = (C.c_void_p * nlev)(*[bufs[2 * l + 1].value for l in range(nlev)])
        rc = mgk.L.mgk_tail_cycle_cs_f64(mgk.ctx, C.byref(g), nlev, nn, None, None, cta, dta, scale, cscale, v0, v1, db, du, None)
    else:
        k7 = mgk.coef([v for ct, _ in tabs for v in list(ct[0]) + [0.0, 0.0]])
        di = mgk.coef([dt[0] for _, dt in tabs])
        rc = mgk.L.mgk_tail_cycle_cs_f64(mgk.ctx, C.byref(g), nlev, nn, k7, di, None, None, scale, cscale, v0, v1, db, du, None)
    mgk._chk(rc)
    got = mgk.from_field(g, du).reshape(n0, n0)
    assert np.array_equal(_bits(got), _bits(want)), f"max diff {np.abs(got - want).max()}"
    for p in [db, du] + bufs:
        mgk.free(p)


TAIL32_CASES = [(15, 4, 3, 3), (15, 3, 2, 1), (15, 2, 1, 4), (15, 1, 0, 3), (7, 3, 3, 3), (7, 2, 2, 2), (7, 1, 0, 1), (3, 2, 1, 3),
                (3, 1, 0, 2), (15, 4, 0, 2)]


@pytest.mark.parametrize("n0,nlev,v0,v1", TAIL32_CASES)
def test_tail_cycle_f32_bit_exact(mgk, orc, n0, nlev, v0, v1):
    """mgk_tail_cycle_f32 (3-D, the fp32 coarse tail of the mixed-precision cycle) against the same levels stepped with the oracle's
    fp32 forms (jacobi32 / residual32 / restrict32 / prolong_add32: coefficients, 1/diag and scale rounded to float once), bit for
    bit.  Random distinct coefficients per level, so a swapped neighbour or a wrong level's constants shows"""
    rng = np.random.default_rng(6000 + n0 + 10 * nlev + v0 + v1)
    ns = [n0]
    for _ in range(nlev - 1):
        ns.append((ns[-1] - 1) // 2)
    scale = 0.8
    As = []
    for n in ns:
        a = rng.uniform(0.5, 1.5, 7) * (n + 1) ** 2
        a[3] = -(a[:3].sum() + a[4:].sum()) * rng.uniform(1.0, 1.2)
        As.append(a)
    b0 = rng.uniform(-1.0, 1.0, n0 ** 3).astype(np.float32)
    want = _tail_ref(ns, b0,
                     lambda l, b, u: orc.jacobi32(ns[l], As[l], scale, b, u),
                     lambda l, b: orc.jacobi32(ns[l], As[l], scale, b, np.zeros_like(b), zero_guess=True),
                     lambda l, b, u: orc.residual32(ns[l], As[l], b, u),
                     lambda l, r: orc.restrict32(ns[l], r),
                     lambda l, uc, uf: orc.prolong_add32(ns[l], uc, uf), v0, v1)
    g = mgk.geom32(n0)
    db, du = mgk.to_field32(g, b0), mgk.field32(g)
    mgk._chk(mgk.L.mgk_memset0(mgk.ctx, du, 4 * g.total, None))
    nn = (C.c_int * nlev)(*ns)
    k7 = mgk.coef([v for a in As for v in a])
    di = mgk.coef([1.0 / a[3] for a in As])
    mgk._chk(mgk.L.mgk_tail_cycle_f32(mgk.ctx, C.byref(g), nlev, nn, k7, di, scale, v0, v1, db, du, None))
    got = mgk.from_field32(g, du)
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"max diff {np.abs(got - want).max()}"
    mgk.free(db)
    mgk.free(du)


@pytest.mark.parametrize("n", [3, 63, 255, 2047])
def test_row_table_operator_modes(mgk, n):
    """mgk_rowcoef_f64, the stretched-mesh operator of the drop-in's MatMult / KSPSolve: mode 0 (Jacobi sweep with dtab), 1 (b - A u)
    and 4 (A u) exact against the row-table statement; ghosts and padding of the output stay zero"""
    rng = np.random.default_rng(6100 + n)
    ct, dt = _rt_tables(rng, n)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    g = mgk.geom(2, n)
    du, db, dout = mgk.to_field(g, u.ravel()), mgk.to_field(g, b.ravel()), mgk.field(g)
    dct, ddt = mgk.upload(ct.ravel()), mgk.upload(dt)
    for mode, want in ((0, _rt_jacobi(ct, b, u, 0.8)), (1, b - _rt_apply(ct, u)), (4, _rt_apply(ct, u))):
        mgk._chk(mgk.L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
        mgk._chk(mgk.L.mgk_rowcoef_f64(mgk.ctx, C.byref(g), mode, dct, ddt if mode == 0 else None, 0.8, None if mode == 4 else db, du, dout, None))
        mgk.sync()
        assert np.array_equal(_bits(mgk.raw_field(g, dout)), _bits(_padded(g, want, 0.0))), f"mode {mode}"
    for p in (du, db, dout, dct, ddt):
        mgk.free(p)


@pytest.mark.parametrize("dim,n", [(3, 7), (3, 63), (3, 127), (2, 255), (2, 2047)])
def test_sweep_over_plane_ranges(mgk, orc, dim, n):
    """mgk_jacobi_range_f64 (the slab solver's interior-first sweep): the inner planes (3-D) / rows (2-D), then the two boundary ones,
    equal the oracle's whole sweep bit for bit; an empty range is refused"""
    rng = np.random.default_rng(6200 + 10 * n + dim)
    As = orc.level_stencil(dim, n + 2, 0)[0]
    dinv = 1.0 / As[3 if dim == 3 else 2]
    u, b = rng.uniform(-1, 1, n ** dim), rng.uniform(-1, 1, n ** dim)
    g = mgk.geom(dim, n)
    du, db, dout = mgk.to_field(g, u), mgk.to_field(g, b), mgk.field(g)
    want = orc.jacobi(dim, n, As, 0.8, b, u)
    try:
        for zc in (-1, 3):
            mgk.L.mgk_set_tuning(-1, zc)
            mgk._chk(mgk.L.mgk_memset0(mgk.ctx, dout, 8 * g.total, None))
            for z0, z1 in ((1, n - 1), (0, 1), (n - 1, n)):
                mgk._chk(mgk.L.mgk_jacobi_range_f64(mgk.ctx, C.byref(g), mgk.coef(As), dinv, 0.8, db, du, dout, z0, z1, None))
            assert np.array_equal(mgk.from_field(g, dout), want), f"zc={zc}"
    finally:
        mgk.L.mgk_set_tuning(-1, -1)
    assert mgk.L.mgk_jacobi_range_f64(mgk.ctx, C.byref(g), mgk.coef(As), dinv, 0.8, db, du, dout, 2, 2, None) != 0
    for p in (du, db, dout):
        mgk.free(p)


@pytest.mark.parametrize("n,cuts", [(31, (0, 9, 31)), (63, (0, 20, 41, 63)), (127, (0, 64, 127))])
def test_two_sweeps_on_z_slabs(mgk, orc, n, cuts):
    """mgk_jacobi2_slab_f64: every z-slab [z0, z1) of a whole n^3 grid, given its neighbours' planes the way the halo exchange delivers
    them (ghost planes of u and b; far: lo = plane z0 - 2, hi = plane z1 + 1 of u), reproduces the oracle's two sweeps on its planes
    bit for bit, in the plane ranges of the slab solver (interior first)"""
    rng = np.random.default_rng(6300 + n)
    As = orc.level_stencil(3, n + 2, 0)[0]
    dinv = 1.0 / As[3]
    u, b = rng.uniform(-1, 1, n ** 3), rng.uniform(-1, 1, n ** 3)
    want = orc.jacobi(3, n, As, 0.8, b, orc.jacobi(3, n, As, 0.8, b, u)).reshape(n, n, n)
    U, B = u.reshape(n, n, n), b.reshape(n, n, n)

    def slab(g, W, z0):
        raw = np.zeros(g.total)
        for k in range(-1, g.nz + 1):
            if 0 <= z0 + k < n:
                for i in range(n):
                    o = g.org + k * g.plane + i * g.pitch
                    raw[o:o + n] = W[z0 + k, i]
        return mgk.upload(raw)
    for s in range(len(cuts) - 1):
        z0, z1 = cuts[s], cuts[s + 1]
        nz, has_lo, has_hi = z1 - z0, int(z0 > 0), int(z1 < n)
        gs, gfar = mgk.geom(3, n, n, nz), mgk.geom(3, n, n, 2)
        far = np.zeros(gfar.total)
        for k, pl in ((-1, U[z0 - 2] if has_lo else None), (2, U[z1 + 1] if has_hi else None)):
            if pl is not None:
                for i in range(n):
                    o = gfar.org + k * gfar.plane + i * gfar.pitch
                    far[o:o + n] = pl[i]
        us, bs, dfar, out = slab(gs, U, z0), slab(gs, B, z0), mgk.upload(far), mgk.field(gs)
        for a0, a1 in (((2, nz - 2), (0, 2), (nz - 2, nz)) if nz >= 6 else ((0, nz),)):
            mgk._chk(mgk.L.mgk_jacobi2_slab_f64(mgk.ctx, C.byref(gs), C.byref(gfar), mgk.coef(As), dinv, 0.8, bs, us, out, dfar,
                                                has_lo, has_hi, a0, a1, None))
        got = mgk.from_field(gs, out).reshape(nz, n, n)
        assert np.array_equal(got, want[z0:z1]), f"slab {s}: planes {np.unique(np.nonzero(got != want[z0:z1])[0]).tolist()}"
        for p in (us, bs, dfar, out):
            mgk.free(p)
