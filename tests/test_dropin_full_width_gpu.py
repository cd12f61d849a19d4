"""The reference's unmodified driver over the PETSc-surface drop-in at the sizes README and BASELINE quote it at (2049^2, 4097^2), with
the default environment: KSPSolve's paired sweeps (n >= MGPETSC_PAIR_MIN_N = 2047 by default), the three-sweep passes, the recorded
coarse tail, KEEP_R and the lazy temporaries together -- the path tests/test_petsc_shim_gpu.py reaches only at npts <= 513 or with
the pairing threshold forced down.  Also the generic CSR path (MGPETSC_NO_RECOGNITION=1) past one grid-stride pass of its kernels
(2047^2 > 2^21 rows), the stretched meshes and PCMG at 2049^2.  Same bar as test_unmodified_reference_driver_on_the_gpu: iteration
count, rData to 1e-12, uData bit for bit, eData to 1e-12, and the KSPView line that names the operator the drop-in recognised."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDRV = os.path.join(ROOT, "oracle", "_ref", "poisson")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not os.path.exists(REFDRV), reason="oracle/_ref/poisson absent: __graft_entry__.build() links it only "
                                 "where the reference tree exists; the binary then travels with the tree")]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _numbers(path):
    """whitespace-separated numbers of an output file (uData.dat at 4097^2 holds 16.8 M lines: np.fromfile, not str.split)"""
    return np.fromfile(str(path), dtype=np.float64, sep=" ")


def _run(tmp_path, opts, extra_env=None):
    (tmp_path / "poisson.in").write_text("# options of the reference driver (same keys as its poisson.in)\n" + opts)
    env = dict(os.environ)
    for k in [k for k in env if k.startswith("MGPETSC_")]:         # the default environment of the drop-in
        del env[k]
    env.update(extra_env or {})
    p = subprocess.run([REFDRV], cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    it = int(re.search(r"Number of iterations:\s+(\d+)", p.stdout).group(1))
    return it, _numbers(tmp_path / "rData.dat"), _numbers(tmp_path / "uData.dat"), _numbers(tmp_path / "eData.dat"), p.stdout


def _check(it, rdat, u, e, ref, eref, npts):
    assert it == ref["iters"]
    want = ref["rnorm"] / ref["rnorm"][0]                # solver.c:1554-1557 normalises by rnorm[0]
    assert rdat.size == it + 1
    assert np.max(np.abs(rdat - want) / want) <= 1e-12
    assert u.size == (npts - 2) ** 2
    assert np.array_equal(u, ref["u"])                   # %.16e round-trips a double
    assert np.allclose(e, eref, rtol=1e-12, atol=0)


def _opts(npts, levels, mesh=0, cycle=0, iters=1000, extra=""):
    return (f"-npts {npts}\n-mesh {mesh}\n-iter {iters}\n-grids {levels}\n-levels {levels}\n-cycle {cycle}\n-map 2\n-v 3,3\n-moreNorm 0\n"
            + extra)


@pytest.mark.parametrize("npts,levels", [(2049, 11), (4097, 12)])
def test_reference_driver_at_full_width_default_environment(orc, tmp_path, npts, levels):
    """-cycle 0, Richardson 0.8 + Jacobi, every option of the drop-in at its default"""
    it, rdat, u, e, out = _run(tmp_path, _opts(npts, levels, extra="-pc_type jacobi\n-ksp_richardson_scale 0.8\n"))
    ref = orc.vcycle(2, npts, levels, 3, 3, maxiter=1000, scale=0.8, use_csr=0)
    _check(it, rdat, u, e, ref, orc.error_norms(2, npts, ref["u"]), npts)
    assert "matrix-free 5-point stencil" in out


def test_reference_driver_generic_csr_path_past_one_grid_stride_pass(orc, tmp_path):
    """MGPETSC_NO_RECOGNITION=1 at 2049^2: the assembled operators run on k_csr_mult (4.19 M rows, two grid-stride passes) and the
    vectors on the flat kernels (padded fields of 4.2 M doubles); -iter 30 bounds the run, the oracle gets the same bound"""
    npts, levels, iters = 2049, 11, 30
    it, rdat, u, e, out = _run(tmp_path, _opts(npts, levels, iters=iters, extra="-pc_type jacobi\n-ksp_richardson_scale 0.8\n"),
                               {"MGPETSC_NO_RECOGNITION": "1"})
    ref = orc.vcycle(2, npts, levels, 3, 3, maxiter=iters, scale=0.8, use_csr=0)
    _check(it, rdat, u, e, ref, orc.error_norms(2, npts, ref["u"]), npts)
    assert "assembled AIJ (generic CSR kernel)" in out


@pytest.mark.parametrize("mesh", [1, 2])
def test_reference_driver_stretched_meshes_at_full_width(orc, tmp_path, mesh):
    """-mesh 1 / 2 at 2049^2: the row-table operators (recognised at MatAssemblyEnd) against the oracle's CSR leg on the same mesh"""
    npts, levels = 2049, 11
    it, rdat, u, e, out = _run(tmp_path, _opts(npts, levels, mesh=mesh, extra="-pc_type jacobi\n-ksp_richardson_scale 0.8\n"))
    ref = orc.vcycle(2, npts, levels, 3, 3, maxiter=1000, scale=0.8, use_csr=1, mesh=mesh)
    _check(it, rdat, u, e, ref, orc.error_norms_mesh(npts, mesh, ref["u"]), npts)
    assert "row-dependent coefficients" in out


def test_reference_driver_pcmg_at_full_width(orc, tmp_path):
    """-cycle 8 (outer Richardson + PCMG V-cycle, Richardson 0.8 + Jacobi on every level and on the coarse grid) at 2049^2"""
    npts, levels = 2049, 11
    lv = ("-mg_levels_ksp_type richardson\n-mg_levels_pc_type jacobi\n-mg_levels_ksp_max_it 3\n"
          "-mg_coarse_ksp_type richardson\n-mg_coarse_pc_type jacobi\n-mg_coarse_ksp_max_it 3\n"
          "-mg_levels_ksp_richardson_scale 0.8\n-mg_coarse_ksp_richardson_scale 0.8\n")
    it, rdat, u, e, out = _run(tmp_path, _opts(npts, levels, cycle=8, iters=400, extra=lv))
    ref = orc.pcmg(2, npts, levels, 3, 3, maxiter=400, scale=0.8)
    assert it < 400
    _check(it, rdat, u, e, ref, orc.error_norms(2, npts, ref["u"]), npts)
    assert "Petsc-V-Cycle" in out and "type: mg" in out
