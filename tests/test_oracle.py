"""CPU tests (run everywhere): the oracle against the pins we have.

The reference ships no tests or golden vectors and its floating-point work lives in PETSc, which is
not installed.  Pins available: (1) the reference-run outputs recorded in SURVEY.md
8(c2) for the integer half (tests/golden/survey_c2.json), (2) the closed-form discrete-eigenvector
known answer, (3) bit-equality of the two independent restatements inside the oracle (assembled AIJ
path following solver.c's MatSetValue loops vs matrix-free stencils)."""
import json
import math
import os

import numpy as np
import pytest

from oracle import Oracle

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "survey_c2.json")))


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _maps(orc, npts, grids, levels, style, procs, l):
    tot = orc.L.mgo_level_total_2d(npts, grids, levels, l)
    glob = np.zeros(3 * tot, dtype=np.int32)
    grid = np.zeros(tot, dtype=np.int32)
    ranges = np.zeros(procs + 1, dtype=np.int32)
    rc = orc.L.mgo_mapping_2d(npts, grids, levels, style, procs, l, glob.ctypes.data, grid.ctypes.data, ranges.ctypes.data)
    assert rc == 0
    return glob.reshape(tot, 3), grid, ranges


def test_integer_half_against_survey_observations(orc):
    c = GOLD["case_npts17"]
    for l in range(2):
        n = orc.L.mgo_grid_n(c["npts"], l)
        assert n == c["level_n"][l]
        glob, grid, ranges = _maps(orc, c["npts"], c["grids"], c["levels"], c["map"], c["procs"], l)
        assert list(ranges) == c["ranges"][l]
        assert np.array_equal(grid, np.arange(n * n))                      # lexicographic
        assert np.array_equal(glob[:, 0], np.repeat(np.arange(n), n))      # i = row
        assert np.array_equal(glob[:, 1], np.tile(np.arange(n), n))        # j = column
        assert orc.level_stencil(2, c["npts"], l)[1] == c["h"][l]
    w = np.zeros(9)
    orc.L.mgo_restriction_stencil(w.ctypes.data)
    assert list(w) == c["res0"] and w.sum() == 1.0
    orc.L.mgo_prolongation_stencil(w.ctypes.data)
    assert list(w) == c["pro0"] and w.sum() == 4.0
    assert orc.L.mgo_mesh_h(2, 17) == c["mesh_h"]

    c = GOLD["case_npts129"]
    for l, size in enumerate(c["level_sizes"]):
        assert orc.L.mgo_level_total_2d(c["npts"], c["grids"], c["levels"], l) == size
    r = np.zeros(9, dtype=np.int32)
    orc.L.mgo_get_ranges(16129, 8, r.ctypes.data)
    assert list(r[:3]) == c["ranges_level0_head"] and r[-1] == c["ranges_level0_last"]
    orc.L.mgo_get_ranges(9, 8, r.ctypes.data)
    assert list(r) == c["ranges_level5"]


@pytest.mark.parametrize("npts,levels", [(9, 2), (17, 3), (33, 5)])
@pytest.mark.parametrize("procs", [1, 2, 4, 8])
def test_one_grid_per_level_all_styles_coincide(orc, npts, levels, procs):
    """F7: with -grids == -levels the three -map styles give the same lexicographic map and ranges."""
    for l in range(levels):
        ref = _maps(orc, npts, levels, levels, 0, procs, l)
        n = orc.L.mgo_grid_n(npts, l)
        assert np.array_equal(ref[1], np.arange(n * n))
        for style in (1, 2):
            got = _maps(orc, npts, levels, levels, style, procs, l)
            for a, b in zip(ref, got):
                assert np.array_equal(a, b)
        assert ref[2][-1] == n * n and np.all(np.diff(ref[2]) >= 0)
        sizes = np.diff(ref[2])
        assert sizes.max() - sizes.min() <= 1


@pytest.mark.parametrize("style", [0, 1, 2])
@pytest.mark.parametrize("procs", [1, 2, 3, 8])
def test_multi_grid_level_maps_are_consistent(orc, style, procs):
    """levels < grids: the last level holds several grids (src/matbuild.c:27-47).  Every style must give
    a bijection between (grid, i, j) and the global index, with ranges covering all unknowns."""
    npts, grids, levels = 17, 3, 2
    l = 1
    tot = orc.L.mgo_level_total_2d(npts, grids, levels, l)
    assert tot == 7 * 7 + 3 * 3
    glob, grid, ranges = _maps(orc, npts, grids, levels, style, procs, l)
    assert sorted(grid.tolist()) == list(range(tot))
    sizes = [7, 3]
    off = 0
    for lg, n in enumerate(sizes):
        for i in range(n):
            for j in range(n):
                idx = grid[off + i * n + j]
                assert tuple(glob[idx]) == (i, j, 1 + lg)
        off += n * n
    assert ranges[0] == 0 and ranges[-1] == tot and np.all(np.diff(ranges) >= 0)


def test_assembled_rows_follow_fillJacobians(orc):
    """5-point rows, ascending columns, Dirichlet by dropping neighbours (src/solver.c:239-251)."""
    A = orc.build("A", 2, 9, 0)
    rows = orc.csr_rows(A)
    n, c = 7, 64.0
    assert len(rows) == 49
    cols, vals = rows[0]
    assert list(cols) == [0, 1, 7] and list(vals) == [-4 * c, c, c]
    cols, vals = rows[3 * n + 3]
    assert list(cols) == [17, 23, 24, 25, 31] and list(vals) == [c, c, -4 * c, c, c]
    R = orc.csr_rows(orc.build("R", 2, 9, 0))
    assert len(R) == 9 and all(len(cv[0]) == 9 for cv in R)
    assert list(R[0][0]) == [0, 1, 2, 7, 8, 9, 14, 15, 16]
    P = orc.csr_rows(orc.build("P", 2, 9, 0))
    assert max(len(cv[0]) for cv in P) == 4
    assert list(P[8][0]) == [0] and list(P[8][1]) == [1.0]           # fine (1,1) coincides with coarse (0,0)
    assert list(P[0][1]) == [0.25]                                   # corner fine point: one parent, 1/4


@pytest.mark.parametrize("dim,npts,levels,scale", [(2, 17, 2, 1.0), (2, 17, 2, 0.8), (2, 33, 4, 0.8),
                                                   (2, 129, 7, 0.8), (3, 9, 2, 0.8), (3, 17, 4, 6.0 / 7.0)])
def test_two_restatements_agree_bitwise_and_hit_the_known_answer(orc, dim, npts, levels, scale):
    a = orc.vcycle(dim, npts, levels, 3, 3, maxiter=400, scale=scale, use_csr=1)
    b = orc.vcycle(dim, npts, levels, 3, 3, maxiter=400, scale=scale, use_csr=0)
    assert a["iters"] == b["iters"] < 400
    assert np.array_equal(a["rnorm"], b["rnorm"]) and np.array_equal(a["u"], b["u"])
    h = 1.0 / (npts - 1)
    kat = dim * math.pi ** 2 / ((4 * dim / h ** 2) * math.sin(math.pi * h / 2) ** 2) - 1.0
    err = orc.error_norms(dim, npts, a["u"])
    assert abs(err[0] - kat) <= 5e-7
    # stopping rule of src/solver.c:1530
    assert a["rnorm"][-1] <= 1e-7 * a["bnorm"] < a["rnorm"][-2]


def test_known_answer_and_survey_cycle_counts(orc):
    k = GOLD["kat_error_max"]
    for npts, key in ((17, "npts17"), (129, "npts129")):
        h = 1.0 / (npts - 1)
        kat = 2 * math.pi ** 2 / ((8 / h ** 2) * math.sin(math.pi * h / 2) ** 2) - 1.0
        assert abs(kat - k[key]) <= 1e-8 * k[key] + 1e-12
    g = GOLD["survey_indicative_cycles"]
    r = orc.vcycle(2, 129, 7, 3, 3, maxiter=100, scale=0.8)
    assert r["iters"] == g["npts129_levels7"]["cycles"]
    assert abs(r["rnorm"][1] / r["rnorm"][0] - g["npts129_levels7"]["first_reduction"]) < 1e-4
    r = orc.vcycle(2, 129, 6, 3, 3, maxiter=100, scale=0.8)
    assert r["iters"] == g["npts129_levels6"]["cycles"]
    assert abs(r["rnorm"][1] / r["rnorm"][0] - g["npts129_levels6"]["first_reduction"]) < 1e-4
    assert orc.vcycle(2, 17, 2, 3, 3, maxiter=200, scale=1.0)["iters"] == g["npts17_levels2_scale1"]["cycles"]
    assert orc.vcycle(2, 17, 2, 3, 3, maxiter=200, scale=0.8)["iters"] == g["npts17_levels2_scale08"]["cycles"]


def test_chebyshev_restatements_agree(orc):
    a = orc.vcycle(2, 33, 4, 3, 3, maxiter=100, ksp_type=1, emin=0.2, emax=2.0, use_csr=1)
    b = orc.vcycle(2, 33, 4, 3, 3, maxiter=100, ksp_type=1, emin=0.2, emax=2.0, use_csr=0)
    assert a["iters"] == b["iters"] < 100
    assert np.array_equal(a["rnorm"], b["rnorm"]) and np.array_equal(a["u"], b["u"])


def test_rhs_and_coords_follow_repeated_addition(orc):
    c = orc.coords(17)
    d = 1.0 / 16
    acc = [0.0]
    for _ in range(15):
        acc.append(acc[-1] + d)
    acc.append(1.0)
    assert list(c) == acc
    b = orc.rhs(2, 17).reshape(15, 15)
    PI = 3.14159265358979323846
    assert b[2, 5] == -2 * PI * PI * math.sin(PI * c[6]) * math.sin(PI * c[3])


def test_slab_operators_match_whole_grid(orc):
    """P-way z-slab evaluation with ghost planes == whole-grid evaluation (basis of the multi-GPU path)."""
    rng = np.random.default_rng(0)
    n = 15
    As, _ = orc.level_stencil(3, n + 2, 0)
    u, b = rng.uniform(-1, 1, n ** 3), rng.uniform(-1, 1, n ** 3)
    whole = orc.jacobi(3, n, As, 0.8, b, u)
    U, B = u.reshape(n, n, n), b.reshape(n, n, n)
    cuts = [0, 4, 8, 12, 15]
    parts = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        zlo = np.ascontiguousarray(U[a - 1]) if a > 0 else None
        zhi = np.ascontiguousarray(U[e]) if e < n else None
        parts.append(orc.jacobi(3, n, As, 0.8, np.ascontiguousarray(B[a:e]).ravel(),
                                np.ascontiguousarray(U[a:e]).ravel(), nz=e - a, zlo=zlo, zhi=zhi))
    assert np.array_equal(np.concatenate(parts), whole)


# ---- third restatement: committed scipy.sparse vectors (tests/golden/make_golden.py) ----
from golden_cases import GOLD as NPZ, CYCLE_KEYS, MESH_KEYS, cycle_case, mesh_case

GOLD_RTOL = 1e-12      # bar of BASELINE.json north_star; observed: bit-identical fields


@pytest.mark.parametrize("key", CYCLE_KEYS)
@pytest.mark.parametrize("use_csr", [0, 1])
def test_oracle_cycle_matches_committed_scipy_vectors(orc, key, use_csr):
    g = cycle_case(key)
    r = orc.vcycle(g["dim"], g["npts"], g["levels"], g["v0"], g["v1"], maxiter=g["maxiter"], scale=g["scale"], use_csr=use_csr)
    assert r["iters"] == g["iters"]
    assert abs(r["bnorm"] - g["bnorm"]) <= GOLD_RTOL * g["bnorm"]
    assert np.abs(r["rnorm"] - g["rnorm"]).max() <= GOLD_RTOL * g["rnorm"][0]
    assert np.abs(r["rnorm"] / g["rnorm"] - 1).max() <= 1e-9          # per entry, down to 1e-8 of rnorm[0]
    assert np.abs(r["u"] - g["u"]).max() <= GOLD_RTOL * np.abs(g["u"]).max()
    err = orc.error_norms(g["dim"], g["npts"], r["u"])
    assert np.abs(np.asarray(err) / g["err"] - 1).max() <= 1e-11


@pytest.mark.parametrize("dim,npts", [(2, 17), (2, 33), (2, 129), (3, 9), (3, 17), (3, 33)])
def test_oracle_rhs_matches_committed_vectors(orc, dim, npts):
    assert np.abs(orc.rhs(dim, npts) - NPZ["b0_d%d_n%d" % (dim, npts)]).max() <= 1e-13 * dim * math.pi ** 2


@pytest.mark.parametrize("dim,nf", [(2, 31), (3, 15)])
def test_oracle_operators_match_committed_vectors(orc, dim, nf):
    x, xc, y = NPZ["xfer_d%d_fine" % dim], NPZ["xfer_d%d_coarse" % dim], NPZ["xfer_d%d_base" % dim]
    As = orc.level_stencil(dim, nf + 2, 0)[0]
    assert np.array_equal(orc.restrict(dim, nf, x), NPZ["xfer_d%d_restricted" % dim])
    assert np.array_equal(orc.prolong_add(dim, nf, xc, y.copy()), NPZ["xfer_d%d_prolonged" % dim])
    assert np.array_equal(orc.apply(dim, nf, As, x), NPZ["xfer_d%d_applied" % dim])
    assert np.array_equal(orc.residual(dim, nf, As, y, x), NPZ["xfer_d%d_residual" % dim])


@pytest.mark.parametrize("npts,levels", [(9, 3), (17, 4), (33, 5)])
@pytest.mark.parametrize("procs", [1, 2, 4, 8])
def test_ranges_match_committed_vectors(orc, npts, levels, procs):
    """the committed ranges come from a Python formula (tests/golden/make_golden.py: maps); the reference's own, recorded by
    oracle/ref_record.c (tests/golden/ref_maps.npz), must be the same numbers"""
    import ref_fixtures as RF
    want = NPZ["ranges_n%d_p%d" % (npts, procs)]
    full, ranges_only = RF.load_maps()
    case = (npts, levels, levels, 2, procs)
    recorded = ranges_only[case] if case in ranges_only else full[case]["ranges"]
    assert RF.same_bits(np.asarray(want, dtype=np.int32), recorded)
    for l in range(levels):
        for style in (0, 1, 2):
            _, _, ranges = _maps(orc, npts, levels, levels, style, procs, l)
            assert list(ranges) == list(want[l])


# ---- -cycle 8 (PCMG) restatement: SURVEY 8(f) N4 ----
@pytest.mark.parametrize("dim,npts,levels,scale", [(2, 33, 5, 0.8), (2, 129, 7, 0.8), (2, 17, 2, 1.0), (3, 17, 4, 6.0 / 7.0)])
def test_pcmg_restatement_is_the_vcycle_in_correction_form(orc, dim, npts, levels, scale):
    """Outer Richardson(1) + one PCMG V-cycle per application is algebraically the -cycle 0 iteration written in
    correction form (x += M r): same iterates up to rounding, hence same cycle count and residual history.
    This cross-pins the PCMG restatement (parity unpinned by the reference: PETSc-internal) against the V-cycle."""
    a = orc.vcycle(dim, npts, levels, 3, 3, maxiter=400, scale=scale)
    b = orc.pcmg(dim, npts, levels, 3, 3, maxiter=400, scale=scale)
    c = orc.pcmg(dim, npts, levels, 3, 3, maxiter=400, scale=scale, use_csr=1)
    assert b["iters"] == c["iters"] and np.array_equal(b["rnorm"], c["rnorm"]) and np.array_equal(b["u"], c["u"])
    assert a["iters"] == b["iters"]
    assert np.abs(b["rnorm"] / a["rnorm"] - 1).max() <= 1e-6      # rounding differs between the two forms
    assert np.abs(a["u"] - b["u"]).max() <= 1e-9 * np.abs(a["u"]).max()


def test_icycle_restatement(orc):
    """-cycle 1, one grid: both legs agree bit for bit; 9x9 grid converges to the discrete solution (KAT)."""
    a = orc.icycle(2, 9, maxiter=2000, scale=0.8)
    b = orc.icycle(2, 9, maxiter=2000, scale=0.8, use_csr=1)
    assert a["iters"] == b["iters"] < 2000 and np.array_equal(a["rnorm"], b["rnorm"]) and np.array_equal(a["u"], b["u"])
    h = 1.0 / 8
    kat = 2 * math.pi ** 2 / ((8 / h ** 2) * math.sin(math.pi * h / 2) ** 2) - 1.0
    assert abs(orc.error_norms(2, 9, a["u"])[0] - kat) <= 5e-7
    assert np.all(np.diff(a["rnorm"]) < 0)


@pytest.mark.parametrize("key", MESH_KEYS)
def test_oracle_stretched_mesh_cycle_matches_committed_scipy_vectors(orc, key):
    """-mesh 1/2: the oracle's assembled leg against the scipy.sparse restatement (coordinates and metrics through Python's
    math module: agreement to 1e-12, not bit for bit)"""
    g = mesh_case(key)
    r = orc.vcycle(2, g["npts"], g["levels"], g["v0"], g["v1"], maxiter=g["maxiter"], scale=g["scale"], use_csr=1, mesh=g["mesh"])
    assert r["iters"] == g["iters"]
    assert abs(r["bnorm"] - g["bnorm"]) <= GOLD_RTOL * g["bnorm"]
    assert np.abs(r["rnorm"] - g["rnorm"]).max() <= 1e-11 * g["rnorm"][0]
    assert np.abs(r["u"] - g["u"]).max() <= 1e-11 * np.abs(g["u"]).max()
    err = orc.error_norms_mesh(g["npts"], g["mesh"], r["u"])
    assert np.abs(np.asarray(err) / g["err"] - 1).max() <= 1e-9


# ---- fp32 leg (mgo_f32.c): thin-grid forms, an independent binary32 restatement, float64 forward-error bounds ----
U32 = 2.0 ** -24                      # unit roundoff of IEEE binary32 (round to nearest)
THIN32 = [(7, 7, 7), (15, 15, 3), (31, 31, 5), (15, 7, 9), (31, 11, 3), (63, 3, 7)]     # (nx, ny, nz): cubes, thin slabs, ny != nx


def _rand32(rng, *shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


def _coef_rand(rng):
    """seven distinct coefficients of mixed sign (the level stencils have six equal off-diagonal ones, under which a swapped
    neighbour would go unseen), diagonal dominant"""
    As = rng.uniform(0.5, 2.0, 7) * rng.choice([-1.0, 1.0], 7)
    As[3] = -8.0
    return As


def _shift(x, axis, d):
    """x moved by d along axis with zero fill: _shift(x, 0, 1)[k] = x[k - 1]"""
    y = np.zeros_like(x)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if d > 0:
        dst[axis], src[axis] = slice(d, None), slice(None, -d)
    else:
        dst[axis], src[axis] = slice(None, d), slice(-d, None)
    y[tuple(dst)] = x[tuple(src)]
    return y


# the seven terms of a row in the canonical order {(k-1), (i-1), (j-1), C, (j+1), (i+1), (k+1)}: (axis, shift) of x
_TERMS = [(0, 1), (1, 1), (2, 1), None, (2, -1), (1, -1), (0, -1)]


def _np_apply32(As32, x):
    """A x in binary32, canonical order, one rounding per multiply and per add (numpy float32 arithmetic: no FMA, no wider
    accumulator).  Terms that fall outside the grid are skipped, not added as zeros, as in mgo_f32.c."""
    s = np.zeros_like(x)
    for q, t in enumerate(_TERMS):
        if t is None:
            s = s + As32[q] * x
            continue
        axis, d = t
        inside = _shift(np.ones_like(x, dtype=bool), axis, d)
        s = np.where(inside, s + As32[q] * _shift(x, axis, d), s)
    return s


def _np_jacobi32(As, scale, b, u, zero_guess=False):
    As32, dinv = Oracle.coef32(As)
    sc = np.float32(scale)
    if zero_guess:
        return sc * (b * dinv)
    return u + sc * ((b - _np_apply32(As32, u)) * dinv)


_W1 = np.array([0.25, 0.5, 0.25], dtype=np.float32)
_W2 = np.array([0.0625, 0.125, 0.0625, 0.125, 0.25, 0.125, 0.0625, 0.125, 0.0625], dtype=np.float32)


def _np_restrict32(rf, nzc):
    nzf, nyf, nxf = rf.shape
    nyc, nxc = (nyf - 1) // 2, (nxf - 1) // 2
    s = np.zeros((nzc, nyc, nxc), dtype=np.float32)
    for dk in range(3):
        for di in range(3):
            for dj in range(3):
                w = _W1[dk] * _W2[di * 3 + dj]
                pl = np.zeros((nzc, nyc, nxc), dtype=np.float32)
                ks = [k for k in range(nzc) if 2 * k + dk < nzf]
                pl[ks] = rf[[2 * k + dk for k in ks]][:, di:di + 2 * nyc:2, dj:dj + 2 * nxc:2]
                inside = np.zeros((nzc, 1, 1), dtype=bool)
                inside[ks] = True
                s = np.where(inside, s + w * pl, s)
    return s


def _axis_parents(nf, nc):
    """for every fine index: its (up to two) coarse parents in ascending order, whether each exists, and its weight"""
    f = np.arange(nf)
    odd = (f & 1) == 1
    c0 = np.where(odd, (f - 1) // 2, f // 2 - 1)
    c1 = np.where(odd, c0, f // 2)
    w = np.where(odd, np.float32(1.0), np.float32(0.5)).astype(np.float32)
    ok0 = (c0 >= 0) & (c0 < nc)
    ok1 = ~odd & (c1 >= 0) & (c1 < nc)
    return [(np.clip(c0, 0, max(nc - 1, 0)), ok0), (np.clip(c1, 0, max(nc - 1, 0)), ok1)], w


def _np_prolong_add32(uc, uf):
    nzf, nyf, nxf = uf.shape
    nzc, nyc, nxc = uc.shape
    pk, wk = _axis_parents(nzf, nzc)
    pi, wi = _axis_parents(nyf, nyc)
    pj, wj = _axis_parents(nxf, nxc)
    w = wk[:, None, None] * (wi[None, :, None] * wj[None, None, :])
    s = np.zeros_like(uf)
    for ck, okk in pk:                 # kc ascending, then ic, then jc: the loop order of mgo_st_prolong_add_f32
        for ci, oki in pi:
            for cj, okj in pj:
                ok = okk[:, None, None] & oki[None, :, None] & okj[None, None, :]
                if uc.size:
                    v = uc[ck[:, None, None], ci[None, :, None], cj[None, None, :]]
                    s = np.where(ok, s + w * v, s)
    return uf + s


def _f64_apply_abs(As32, x):
    """float64 values of sum_q a_q x_q and of sum_q |a_q x_q| (the products of binary32 operands are exact in float64)"""
    a64, x64 = As32.astype(np.float64), x.astype(np.float64)
    t, m = np.zeros_like(x64), np.zeros_like(x64)
    for q, sh in enumerate(_TERMS):
        v = x64 if sh is None else _shift(x64, *sh)
        t += a64[q] * v
        m += np.abs(a64[q] * v)
    return t, m


@pytest.mark.parametrize("n", [1, 3, 7, 15])
def test_fp32_thin_forms_with_nz_equal_n_are_the_cube_forms(orc, n):
    """the cube entry points (what mgo_vcycle_mixed calls) and the thin ones with nx = ny = nz: bit for bit"""
    rng = np.random.default_rng(8800 + n)
    As = orc.level_stencil(3, n + 2, 0)[0]
    u, b = _rand32(rng, n ** 3), _rand32(rng, n ** 3)
    for zg in (False, True):
        assert np.array_equal(orc.jacobi32(n, As, 6.0 / 7.0, b, u, zero_guess=zg), orc.jacobi32(n, As, 6.0 / 7.0, b, u, zero_guess=zg, nz=n, ny=n))
    assert np.array_equal(orc.residual32(n, As, b, u), orc.residual32(n, As, b, u, nz=n))
    if n >= 3:
        nc = (n - 1) // 2
        uc = _rand32(rng, nc ** 3)
        assert np.array_equal(orc.restrict32(n, u), orc.restrict32(n, u, nzf=n, nzc=nc))
        assert np.array_equal(orc.prolong_add32(n, uc, u), orc.prolong_add32(n, uc, u, nzf=n, nzc=nc))


@pytest.mark.parametrize("nx,ny,nz", [(7, 7, 3), (15, 7, 5), (15, 15, 1)])
def test_fp32_thin_forms_are_a_cube_with_zero_planes_beyond(orc, nx, ny, nz):
    """Dirichlet at z = nz: the thin sweep / residual equal the first nz planes of the same operation on a taller grid whose
    planes nz, nz+1, .. hold zeros (a zero neighbour adds +0.0 where the thin form adds nothing: same bits for these data)"""
    rng = np.random.default_rng(8900 + nx + ny + nz)
    As = _coef_rand(rng)
    u, b = _rand32(rng, nz, ny, nx), _rand32(rng, nz, ny, nx)
    tall = nz + 2
    U, B = np.zeros((tall, ny, nx), np.float32), np.zeros((tall, ny, nx), np.float32)
    U[:nz], B[:nz] = u, b
    N = nx * ny * nz
    got = orc.jacobi32(nx, As, 0.8, b.ravel(), u.ravel(), nz=nz, ny=ny)
    assert np.array_equal(got, orc.jacobi32(nx, As, 0.8, B.ravel(), U.ravel(), nz=tall, ny=ny)[:N])
    got = orc.residual32(nx, As, b.ravel(), u.ravel(), nz=nz, ny=ny)
    assert np.array_equal(got, orc.residual32(nx, As, B.ravel(), U.ravel(), nz=tall, ny=ny)[:N])


@pytest.mark.parametrize("nx,ny,nz", THIN32)
def test_fp32_leg_equals_a_binary32_restatement(orc, nx, ny, nz):
    """The fp32 leg against an independent restatement in numpy float32 (IEEE binary32, one rounding per operation, no FMA): same
    canonical order, so the same bits.  Random distinct coefficients: a swapped neighbour, a lost term, a wider accumulator or a
    reordered sum in the oracle makes this fail."""
    rng = np.random.default_rng(9000 + nx * ny + nz)
    As = _coef_rand(rng)
    sc = 6.0 / 7.0
    u, b = _rand32(rng, nz, ny, nx), _rand32(rng, nz, ny, nx)
    kw = dict(nz=nz, ny=ny)
    for zg in (False, True):
        assert np.array_equal(orc.jacobi32(nx, As, sc, b.ravel(), u.ravel(), zero_guess=zg, **kw), _np_jacobi32(As, sc, b, u, zg).ravel())
    assert np.array_equal(orc.residual32(nx, As, b.ravel(), u.ravel(), **kw), (b - _np_apply32(Oracle.coef32(As)[0], u)).ravel())
    nzc = (nz - 1) // 2
    assert np.array_equal(orc.restrict32(nx, u.ravel(), nzf=nz, nzc=nzc, nyf=ny), _np_restrict32(u, nzc).ravel())
    nzc1 = nz // 2                                             # a slab's last coarse plane without its third fine plane
    assert np.array_equal(orc.restrict32(nx, u.ravel(), nzf=nz, nzc=nzc1, nyf=ny), _np_restrict32(u, nzc1).ravel())
    uc = _rand32(rng, nzc, (ny - 1) // 2, (nx - 1) // 2)
    assert np.array_equal(orc.prolong_add32(nx, uc.ravel(), u.ravel(), nzf=nz, nzc=nzc, nyf=ny), _np_prolong_add32(uc, u).ravel())


@pytest.mark.parametrize("nx,ny,nz", THIN32 + [(255, 7, 3)])
def test_fp32_leg_within_its_forward_error_bound(orc, nx, ny, nz):
    """The fp32 leg against the same operations evaluated in float64 from the same binary32 inputs and the binary32-rounded
    coefficients a_q = (float) As[q], d = (float) (1 / As[3]), s = (float) scale.  With u = 2^-24 and gamma_m = m u / (1 - m u):

    sweep  o = u + s*((b - t)*d), t = sum of <= 7 products accumulated left to right.  |t^ - t| <= gamma_7 S, S = sum |a_q x_q|;
           the subtraction, the two multiplications and the final addition add one rounding each, so to first order
           |o^ - o| <= u |u| + gamma_10 |s d| (|b| + S) + O(u^2)  <=  16 u (|u| + |s d| (|b| + S)).
    residual r = b - t:  |r^ - r| <= gamma_8 (|b| + S)  <=  10 u (|b| + S).
    restriction: 27 terms w x with w = 2^-k (the product is exact), accumulated left to right: |e| <= gamma_26 sum |w x| <= 28 u sum |w x|.
    prolongation: <= 8 terms w x (w = 1, 1/2, 1/4, 1/8: exact), sum then one add: |e| <= gamma_8 (|uf| + sum |w uc|) <= 9 u (..).
    float64 evaluation error is ~2^-53 relative, far below these.  A missing or misplaced term (random distinct coefficients) moves
    the result by O(1): it fails the bound.  (The bound does not see a wider accumulator; the binary32 restatement above does.)"""
    rng = np.random.default_rng(9100 + nx * ny + nz)
    As = _coef_rand(rng)
    As32, d32 = Oracle.coef32(As)
    s32 = np.float32(6.0 / 7.0)
    u, b = _rand32(rng, nz, ny, nx), _rand32(rng, nz, ny, nx)
    kw = dict(nz=nz, ny=ny)
    t, S = _f64_apply_abs(As32, u)
    sd = float(s32) * float(d32)
    u64, b64 = u.astype(np.float64), b.astype(np.float64)
    o = orc.jacobi32(nx, As, float(s32), b.ravel(), u.ravel(), **kw).reshape(u.shape)
    ref = u64 + sd * (b64 - t)
    assert np.all(np.abs(o - ref) <= 16 * U32 * (np.abs(u64) + abs(sd) * (np.abs(b64) + S))), "sweep"
    o = orc.jacobi32(nx, As, float(s32), b.ravel(), u.ravel(), zero_guess=True, **kw).reshape(u.shape)
    assert np.all(np.abs(o - sd * b64) <= 3 * U32 * abs(sd) * np.abs(b64)), "zero-guess sweep"
    o = orc.residual32(nx, As, b.ravel(), u.ravel(), **kw).reshape(u.shape)
    assert np.all(np.abs(o - (b64 - t)) <= 10 * U32 * (np.abs(b64) + S)), "residual"
    nzc = (nz - 1) // 2
    if nzc:
        o = orc.restrict32(nx, u.ravel(), nzf=nz, nzc=nzc, nyf=ny).astype(np.float64)
        ref, mag = np.zeros_like(o), np.zeros_like(o)
        nyc, nxc = (ny - 1) // 2, (nx - 1) // 2
        for dk in range(3):
            for di in range(3):
                for dj in range(3):
                    v = float(_W1[dk]) * float(_W2[di * 3 + dj]) * u64[dk:dk + 2 * nzc:2, di:di + 2 * nyc:2, dj:dj + 2 * nxc:2].ravel()
                    ref += v
                    mag += np.abs(v)
        assert np.all(np.abs(o - ref) <= 28 * U32 * mag), "restriction"
        uc = _rand32(rng, nzc, nyc, nxc)
        o = orc.prolong_add32(nx, uc.ravel(), u.ravel(), nzf=nz, nzc=nzc, nyf=ny).reshape(u.shape).astype(np.float64)
        pu = _np_prolong_add32(uc.astype(np.float64), np.zeros_like(u64))          # exact in float64: <= 8 terms of 2^-k x
        pm = _np_prolong_add32(np.abs(uc.astype(np.float64)), np.zeros_like(u64))
        assert np.all(np.abs(o - (u64 + pu)) <= 9 * U32 * (np.abs(u64) + pm)), "prolongation"
