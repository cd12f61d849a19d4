"""CPU tier of the non-symmetric coefficient cases (tests/coef_cases.py).

1. The inputs are what they claim: distinct values, both signs, W != E, diagonal dominance.
2. The fp64 oracle's stencil operators (mgo_st_apply / jacobi / residual / cheby_step, whole grids and z-slabs with ghost planes)
   equal the numpy restatement of the canonical order BIT FOR BIT on such coefficients, and a swapped pair of coefficients in
   the reference changes the result: the reference is pinned before tests/test_distinct_coef_gpu.py leans on it.
3. Completeness: every entry point of include/mgk.h whose parameters name coef, coef7, ctab, ctab_f or dtab is named by
   tests/test_distinct_coef_gpu.py, or exempt here with its reason (reads files only)."""
import os
import re

import numpy as np
import pytest

from coef_cases import (DistinctOracle, dense_field, distinct_coef, distinct_row_tables, np_apply, np_cheby_step, np_residual,
                        np_sweep, np_sweep_zero)
from oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 7, 7), (3, 15, 3), (3, 31, 5), (2, 15, 1), (2, 63, 1)]          # (dim, n, nz)
SCALES = (6.0 / 7.0, 0.8, 1.0)
CHEB = (-0.37, 1.37, 0.21)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("dim", [2, 3])
def test_coefficient_sets_are_distinct_mixed_sign_and_dominant(dim):
    rng = np.random.default_rng(100 + dim)
    m, c = (7, 3) if dim == 3 else (5, 2)
    for _ in range(50):
        As = distinct_coef(rng, dim)
        off = np.delete(As, c)
        assert As.size == m and As[c] == -8.0 and np.unique(As).size == m
        assert (off > 0).any() and (off < 0).any()
        assert np.all((np.abs(off) >= 0.5) & (np.abs(off) < 1.25)) and np.abs(off).sum() < 8.0
    sets = distinct_coef(rng, dim, per_level=6)
    assert len(sets) == 6
    off = np.concatenate([np.delete(a, c) for a in sets])
    assert np.unique(off).size == off.size


def test_row_tables_are_distinct_with_west_unlike_east():
    rng = np.random.default_rng(7)
    for n in (1, 7, 63):
        ct, dt = distinct_row_tables(rng, n)
        assert ct.shape == (n, 5) and dt.shape == (n,)
        assert np.all(ct[:, 1] != ct[:, 3]) and np.all(ct[:, 0] != ct[:, 4])
        assert all(np.unique(row).size == 5 for row in ct)
        off = np.abs(ct[:, [0, 1, 3, 4]])
        assert np.all(ct[:, 2] <= -off.sum(axis=1)) and np.all(ct[:, 2] >= -1.2 * off.sum(axis=1) - 1e-12)
        assert np.array_equal(dt, 1.0 / ct[:, 2])
        assert len({tuple(r) for r in ct}) == n                    # the rows differ from each other too


def test_distinct_oracle_gives_every_level_its_own_set(orc):
    d = DistinctOracle()
    a, h = d.level_stencil(3, 33, 0)
    assert h == orc.level_stencil(3, 33, 0)[1]
    assert np.array_equal(a, d.level_stencil(3, 33, 0)[0])                      # reproducible
    others = [d.level_stencil(3, 33, 1)[0], d.level_stencil(3, 17, 0)[0]]
    assert all(not np.array_equal(a, o) for o in others)
    assert d.level_stencil(2, 33, 0)[0].size == 5 and np.unique(a).size == 7


def _shape(dim, n, nz):
    return (nz, n, n) if dim == 3 else (n, n)


@pytest.mark.parametrize("dim,n,nz", SHAPES)
def test_oracle_equals_the_numpy_restatement_bit_for_bit(orc, dim, n, nz):
    rng = np.random.default_rng(5000 + 10 * n + nz)
    As = distinct_coef(rng, dim)
    sh = _shape(dim, n, nz)
    u, b, pm = dense_field(rng, *sh), dense_field(rng, *sh), dense_field(rng, *sh)
    kw = {"nz": nz} if dim == 3 else {}
    f = lambda a: np.ascontiguousarray(a).ravel()
    assert np.array_equal(orc.apply(dim, n, As, f(u), **kw), f(np_apply(As, u)))
    assert np.array_equal(orc.residual(dim, n, As, f(b), f(u), **kw), f(np_residual(As, b, u)))
    for s in SCALES:
        assert np.array_equal(orc.jacobi(dim, n, As, s, f(b), f(u), **kw), f(np_sweep(As, s, b, u)))
        assert np.array_equal(orc.jacobi(dim, n, As, s, f(b), f(u), zero_guess=True, **kw), f(np_sweep_zero(As, s, b)))
    assert np.array_equal(orc.cheby_step(dim, n, As, f(b), f(u), f(pm), *CHEB, **kw), f(np_cheby_step(As, b, u, pm, *CHEB)))
    # sixty undamped sweeps stay bounded: the repeated-sweep kernels cannot overflow on these operators
    x = u
    for _ in range(60):
        x = np_sweep(As, 1.0, b, x)
    assert np.isfinite(x).all() and np.abs(x).max() < 1.0
    # teeth: the reference itself notices a swapped pair of coefficients
    m = As.size
    for p, q in ((0, m - 1), (1, m - 2), (m // 2 - 1, m // 2 + 1)):
        sw = As.copy()
        sw[p], sw[q] = As[q], As[p]
        assert not np.array_equal(orc.apply(dim, n, sw, f(u), **kw), f(np_apply(As, u))), (p, q)
        assert not np.array_equal(f(np_apply(sw, u)), f(np_apply(As, u))), (p, q)


@pytest.mark.parametrize("n,nz,cut", [(7, 7, (2, 5)), (15, 3, (1, 2)), (31, 5, (0, 3)), (31, 5, (2, 5))])
def test_oracle_slab_forms_equal_the_numpy_restatement(orc, n, nz, cut):
    """the z-slab [z0, z1) of a whole n x n x nz grid with its neighbours' planes as zlo / zhi (None at the grid's faces): the oracle's slab
    forms equal the numpy restatement of the slab, which in turn is the whole grid's result on those planes"""
    rng = np.random.default_rng(6000 + n + nz + cut[0])
    As = distinct_coef(rng, 3)
    u, b, pm = (dense_field(rng, nz, n, n) for _ in range(3))
    z0, z1 = cut
    zlo = np.ascontiguousarray(u[z0 - 1]) if z0 > 0 else None
    zhi = np.ascontiguousarray(u[z1]) if z1 < nz else None
    f = lambda a: np.ascontiguousarray(a).ravel()
    us, bs, ps = u[z0:z1], b[z0:z1], pm[z0:z1]
    kw = dict(nz=z1 - z0, zlo=zlo, zhi=zhi)
    want_apply = np_apply(As, us, zlo, zhi)
    assert np.array_equal(want_apply, np_apply(As, u)[z0:z1])
    assert np.array_equal(orc.apply(3, n, As, f(us), **kw), f(want_apply))
    assert np.array_equal(orc.residual(3, n, As, f(bs), f(us), **kw), f(np_residual(As, bs, us, zlo, zhi)))
    assert np.array_equal(orc.jacobi(3, n, As, 6.0 / 7.0, f(bs), f(us), **kw), f(np_sweep(As, 6.0 / 7.0, bs, us, zlo, zhi)))
    assert np.array_equal(orc.cheby_step(3, n, As, f(bs), f(us), f(ps), *CHEB, **kw), f(np_cheby_step(As, bs, us, ps, *CHEB, zlo, zhi)))
    if zlo is not None and zhi is not None:
        sw = As.copy()
        sw[0], sw[6] = As[6], As[0]
        assert not np.array_equal(orc.apply(3, n, sw, f(us), **kw), f(want_apply))


# ---- completeness gate ----------------------------------------------------------------------------------------------------------
COEF_PARAMS = ("coef", "coef7", "ctab", "ctab_f", "dtab")
GPU_MODULE = os.path.join(ROOT, "tests", "test_distinct_coef_gpu.py")

EXEMPT = {
    "mgk_apply_add_f64": "tests/test_dropin_kernels_gpu.py::test_apply_add_bit_exact draws five independent uniform(-3, 3) coefficients",
    "mgk_tail_cycle_f32": "tests/test_dropin_kernels_gpu.py::test_tail_cycle_f32_bit_exact draws seven distinct coefficients per level",
}


def _coef_entry_points():
    with open(os.path.join(ROOT, "include", "mgk.h")) as fh:
        h = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    out = []
    for name, params in re.findall(r"^\s*(?:const\s+)?\w+\s*\**\s*(mgk_\w+)\s*\(([^;{]*?)\)\s*;", h, re.M | re.S):
        idents = set(re.findall(r"\b\w+\b", params))
        if idents & set(COEF_PARAMS):
            out.append(name)
    return out


def test_header_parse_finds_the_coefficient_taking_entry_points():
    names = _coef_entry_points()
    assert len(names) == len(set(names)) >= 78
    for n in ("mgk_jacobi_f64", "mgk_tail_cycle_cs_f64", "mgk_residual_restrict_2d_rowcoef_f64", "mgk_jacobi_zero_rowcoef_f64",
              "mgk_correct_residual_f64_f32_jz", "mgk_prolong_cheby3_2d_f64", "mgk_jacobi2_slab_f32"):
        assert n in names
    for n in ("mgk_jacobi_zero_f64", "mgk_restrict_fw_f64", "mgk_prolong_add_f64", "mgk_sumsq_f64", "mgk_set_tuning"):
        assert n not in names


def test_every_coefficient_taking_entry_point_has_a_distinct_coefficient_case():
    with open(GPU_MODULE) as fh:
        text = fh.read()
    gap = {n for n in _coef_entry_points() if not re.search(r"\b%s\b" % re.escape(n), text)}
    missing = sorted(gap - set(EXEMPT))
    assert not missing, f"entry points that take stencil coefficients without a case in tests/test_distinct_coef_gpu.py: {missing}"
    stale = sorted(set(EXEMPT) - gap)
    assert not stale, f"exemptions that the module now names or the header no longer declares: {stale}"
    for name, why in EXEMPT.items():
        assert len(why.split()) >= 5, name
