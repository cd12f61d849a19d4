"""The oracle's V-cycle on a right-hand side from the caller (mgo_vcycle_b / mgo_vcycle_mixed_b, Oracle.vcycle(b=)): the reference of
tests/test_rhs_cycle_gpu.py, pinned here on the CPU before anything on the GPU is compared with it.

  * b = None and the manufactured right-hand side passed explicitly are the same computation: same bits, fp64 and mixed.
  * The two restatements inside the oracle (assembled CSR following the reference's MatSetValue loops, matrix-free stencil loops) agree
    bit for bit on rough and on sparse data, as they do on the manufactured mode (test_oracle.py).
  * The loop equals its step primitives: tests/fmg_reference.py's V-cycle, built from Oracle.jacobi / residual / restrict / prolong_add,
    iterated k times gives the bits of vcycle(b=, fixed_cycles=k).
  * An independent statement: the scipy.sparse restatement of tests/golden/make_golden.py on stored right-hand sides
    (tests/golden/vcycle_rhs_golden.npz), with the bars of test_oracle_cycle_matches_committed_scipy_vectors.
Every case that runs to the tolerance first shows, on the oracle's own history, that the stop decision is not near a tie."""
import os

import numpy as np
import pytest

import rhs_cases
from fmg_reference import FmgRef
from oracle import Oracle

GOLD_RTOL = 1e-12            # tests/test_oracle.py
EIG = (0.2, 2.0)
RHS_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vcycle_rhs_golden.npz")


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _scale(dim):
    return 0.8 if dim == 2 else 6.0 / 7.0


def _same_bits(a, b):
    assert a["iters"] == b["iters"]
    assert a["bnorm"] == b["bnorm"]
    assert np.array_equal(a["rnorm"], b["rnorm"])
    assert np.array_equal(a["u"], b["u"])


@pytest.mark.parametrize("dim,npts,levels,use_csr,mesh", [(2, 65, 6, 0, 0), (2, 65, 6, 1, 0), (3, 17, 4, 0, 0), (3, 17, 4, 1, 0),
                                                          (2, 65, 5, 1, 1), (2, 33, 4, 1, 2)])
def test_no_right_hand_side_means_the_manufactured_one(orc, dim, npts, levels, use_csr, mesh):
    b = orc.rhs_mesh(npts, mesh) if mesh else orc.rhs(dim, npts)
    kw = dict(maxiter=400, scale=_scale(dim), use_csr=use_csr, mesh=mesh)
    _same_bits(orc.vcycle(dim, npts, levels, 3, 3, **kw), orc.vcycle(dim, npts, levels, 3, 3, b=b, **kw))
    kw = dict(maxiter=60, ksp_type=1, emin=EIG[0], emax=EIG[1], use_csr=use_csr, mesh=mesh, fixed_cycles=4)
    _same_bits(orc.vcycle(dim, npts, levels, 3, 3, **kw), orc.vcycle(dim, npts, levels, 3, 3, b=b, **kw))


@pytest.mark.parametrize("npts,levels", [(17, 4), (33, 5)])
def test_no_right_hand_side_means_the_manufactured_one_mixed(orc, npts, levels):
    b = orc.rhs(3, npts)
    _same_bits(orc.vcycle_mixed(npts, levels, maxiter=60, scale=6.0 / 7.0), orc.vcycle_mixed(npts, levels, maxiter=60, scale=6.0 / 7.0, b=b))
    _same_bits(orc.vcycle_mixed(npts, levels, scale=6.0 / 7.0, fixed_cycles=3), orc.vcycle_mixed(npts, levels, scale=6.0 / 7.0, fixed_cycles=3, b=b))


def test_a_right_hand_side_of_the_wrong_size_is_refused(orc):
    with pytest.raises(ValueError):
        orc.vcycle(2, 33, 4, b=np.zeros(30 * 31))
    with pytest.raises(ValueError):
        orc.vcycle_mixed(17, 3, b=np.zeros(15 ** 3 + 1))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("family", rhs_cases.FAMILIES)
@pytest.mark.parametrize("dim,npts,levels,cheb", [(2, 129, 7, False), (2, 513, 9, False), (3, 33, 5, False), (3, 65, 6, False),
                                                  (2, 129, 7, True), (3, 33, 5, True)])
def test_two_restatements_agree_bitwise_on_arbitrary_right_hand_sides(orc, family, dim, npts, levels, cheb):
    b = rhs_cases.make(family, dim, npts, seed=1000 + npts)
    kw = dict(ksp_type=1, emin=EIG[0], emax=EIG[1]) if cheb else dict(scale=_scale(dim))
    a = orc.vcycle(dim, npts, levels, 3, 3, maxiter=100, use_csr=1, b=b, **kw)
    s = orc.vcycle(dim, npts, levels, 3, 3, maxiter=100, use_csr=0, b=b, **kw)
    rhs_cases.assert_stop_rule_clear(s, maxiter=100)
    _same_bits(a, s)
    assert s["bnorm"] == np.sqrt(orc.sumsq(b)) and s["rnorm"][0] == s["bnorm"]          # zero guess: r0 = b, nothing manufactured left


@pytest.mark.parametrize("family", rhs_cases.FAMILIES)
@pytest.mark.parametrize("mesh", [1, 2])
def test_stretched_mesh_leg_takes_the_right_hand_side_as_it_is(orc, family, mesh):
    """the CSR leg with -mesh 1/2 has no second restatement inside the oracle (the golden vectors below are its check); here: the given b is
    what it solves for -- r0 = b, and the solution satisfies A u = b to the tolerance with A rebuilt from the oracle's own rows"""
    npts, levels = 129, 7
    b = rhs_cases.make(family, 2, npts, seed=1500 + mesh)
    r = orc.vcycle(2, npts, levels, 3, 3, maxiter=400, scale=0.8, use_csr=1, mesh=mesh, b=b)
    rhs_cases.assert_stop_rule_clear(r, maxiter=400)
    assert r["rnorm"][0] == r["bnorm"] == np.sqrt(orc.sumsq(b))
    A = orc.L.mgo_build_A_mesh(npts, 0, mesh)
    res = b - orc.csr_mult(A, r["u"])
    orc.L.mgo_csr_free(A)
    assert abs(np.sqrt(orc.sumsq(res)) / r["rnorm"][-1] - 1.0) <= 1e-9


@pytest.mark.parametrize("family", rhs_cases.FAMILIES)
@pytest.mark.parametrize("dim,npts,levels,v,k", [(2, 129, 7, (3, 3), 4), (2, 65, 3, (2, 1), 3), (3, 33, 5, (3, 3), 4), (3, 17, 2, (1, 2), 3)])
def test_the_loop_equals_its_step_primitives(orc, family, dim, npts, levels, v, k):
    b = rhs_cases.make(family, dim, npts, seed=2000 + npts)
    f = FmgRef(orc, dim, npts, levels, v, _scale(dim), b0=b)
    u, rn = None, [f.rnorm_of(f.zeros(0))]
    for q in range(k):
        u = f.vcycle(0, b, u, nonzero=q > 0)
        rn.append(f.rnorm_of(u))
    ref = orc.vcycle(dim, npts, levels, v[0], v[1], scale=_scale(dim), fixed_cycles=k, b=b)
    assert ref["iters"] == k
    assert np.array_equal(u, ref["u"])
    assert np.array_equal(np.array(rn), ref["rnorm"])
    assert f.bnorm() == ref["bnorm"]


@pytest.mark.parametrize("family", rhs_cases.FAMILIES)
@pytest.mark.parametrize("npts,levels", [(33, 5), (65, 6)])
def test_mixed_cycle_on_an_arbitrary_right_hand_side_solves_it(orc, family, npts, levels):
    """the fp32 leg has one restatement; on a caller's b its outer loop is the fp64 defect correction of that b: r0 = b, and the history it
    reports is the fp64 residual of the u it returns"""
    b = rhs_cases.make(family, 3, npts, seed=2500 + npts)
    r = orc.vcycle_mixed(npts, levels, maxiter=60, scale=6.0 / 7.0, b=b)
    rhs_cases.assert_stop_rule_clear(r, maxiter=60)
    assert r["rnorm"][0] == r["bnorm"] == np.sqrt(orc.sumsq(b))
    n = npts - 2
    res = orc.residual(3, n, orc.level_stencil(3, npts, 0)[0], b, r["u"])
    assert np.sqrt(orc.sumsq(res)) == r["rnorm"][-1]


# ---- the scipy.sparse restatement on stored right-hand sides ----
GOLDEN_KEYS = ["d2_n33_l5_spikes", "d2_n33_l5_uniform", "d3_n17_l4_spikes", "d3_n17_l4_uniform",
               "mesh1_n33_l4_spikes", "mesh1_n33_l4_uniform", "mesh2_n33_l4_spikes", "mesh2_n33_l4_uniform"]


def _golden_keys():
    if not os.path.exists(RHS_NPZ):
        return []
    with np.load(RHS_NPZ) as z:
        return sorted(k[:-5] for k in z.files if k.endswith("_meta"))


def test_the_stored_right_hand_side_vectors_are_all_there():
    assert _golden_keys() == sorted(GOLDEN_KEYS)
    assert os.path.getsize(RHS_NPZ) < 200 * 1024


# (stretched meshes exist on the assembled leg only)
@pytest.mark.parametrize("key,use_csr", [(k, c) for k in GOLDEN_KEYS for c in (0, 1) if c or not k.startswith("mesh")])
def test_oracle_cycle_on_stored_right_hand_sides_matches_committed_scipy_vectors(orc, key, use_csr):
    with np.load(RHS_NPZ) as z:
        dim, npts, levels, v0, v1, maxiter, iters, mesh = (int(x) for x in z[key + "_meta"])
        scale, bnorm = (float(x) for x in z[key + "_scale"])
        b, u, rnorm = z[key + "_b"], z[key + "_u"], z[key + "_rnorm"]
    assert np.count_nonzero(b) >= 7 and b.min() < 0.0 < b.max()
    r = orc.vcycle(dim, npts, levels, v0, v1, maxiter=maxiter, scale=scale, use_csr=use_csr, mesh=mesh, b=b)
    rhs_cases.assert_stop_rule_clear(r, maxiter=maxiter)
    assert r["iters"] == iters
    assert abs(r["bnorm"] - bnorm) <= GOLD_RTOL * bnorm
    assert np.abs(r["rnorm"] - rnorm).max() <= GOLD_RTOL * rnorm[0]
    assert np.abs(r["rnorm"] / rnorm - 1).max() <= 1e-9
    assert np.abs(r["u"] - u).max() <= GOLD_RTOL * np.abs(u).max()
