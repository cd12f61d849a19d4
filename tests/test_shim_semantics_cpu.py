"""CPU tier: the PETSc-surface drop-in's host logic (petsc_shim.c) linked against the host-memory mock of the kernel ABI
(tests/mock_mgk.cpp) as a shared library and driven through ctypes -- the lazy temporaries in call orders the reference's loop does not
use, and the adoption rule of the speculative sweep (tests/shim_semantics.py; the same functions run on the GPU tier over the real
libmgpetsc.so).  Test infrastructure: nothing under multigrid_petsc_amd/ links the mock."""
import os
import shutil
import subprocess
import sys

import pytest

from shim_semantics import MODES, lazy_stats, random_programs_went_the_way_of_the_mode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "_san")


@pytest.fixture(scope="module")
def mock_shim():
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    os.makedirs(OUT, exist_ok=True)
    inc = "-I" + os.path.join(ROOT, "include")
    so = os.path.join(OUT, "libmgpetsc_mock.so")
    objs = []
    for cc, std, src, obj in (("g++", "-std=c++17", os.path.join(ROOT, "tests", "mock_mgk.cpp"), "mock_mgk_pic.o"),
                              ("gcc", "-std=c99", os.path.join(ROOT, "multigrid_petsc_amd", "csrc", "petsc_shim.c"), "petsc_shim_pic.o")):
        o = os.path.join(OUT, obj)
        p = subprocess.run([cc, std, "-O1", "-g", "-fPIC", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L", inc, "-c", src, "-o", o],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    # -Bsymbolic: the library's own mgk_* / PETSc-surface definitions, whatever else the process has loaded
    p = subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return so


def _check(so, which, *more, env=None):
    # a process of its own: the drop-in ends the process on a fatal error, and the test process may hold the real libraries
    # (env: the drop-in's switches for that process -- they are read once and cached)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_semantics.py"), so, which] + list(more), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0 and "SEMANTICS_OK " + which in p.stdout, (p.returncode, p.stdout[-3000:])
    return p.stdout


def test_lazy_temporaries_keep_petsc_semantics_on_the_mock(mock_shim):
    _check(mock_shim, "lazy")


def test_speculative_sweep_adoption_rule_on_the_mock(mock_shim):
    _check(mock_shim, "spec")


def test_residual_left_deferred_by_the_norm_pass_on_the_mock(mock_shim):
    _check(mock_shim, "keepr")


def test_recorded_coarse_subcycle_keeps_petsc_semantics_on_the_mock(mock_shim):
    _check(mock_shim, "tailrec")


def test_deferred_values_around_the_recorder_on_the_mock(mock_shim):
    """a Chebyshev solve on a right-hand side an open recording has taken; P b deferred, then b overwritten while a finished log names it"""
    _check(mock_shim, "recorder")


def test_pcmg_level_vectors_after_the_tail_launch_on_the_mock(mock_shim):
    _check(mock_shim, "pcmgtail")


def test_richardson_with_lu_is_damped_on_the_mock(mock_shim):
    _check(mock_shim, "lu")


def test_nonsymmetric_operators_keep_petsc_semantics_on_the_mock(mock_shim):
    """five distinct coefficients / row tables with W != E through MatSetValue: recognised, and every value that of dense numpy"""
    _check(mock_shim, "nonsym")


def test_reference_streams_replayed_into_the_drop_in_on_the_mock(mock_shim):
    """the reference's own recorded MatSetValue / VecSetValue calls (tests/golden/ref_assembly.npz) in their own order: recognised operators,
    MatMult equal to the canonical product bit for bit, b[0] exact; see tests/shim_semantics.py: reference_streams"""
    _check(mock_shim, "refstreams")


def test_random_programs_of_petsc_calls_keep_petsc_semantics_on_the_mock(mock_shim):
    """random_programs_keep_petsc_semantics: 25 programs of up to 60 calls (seed 1); round 3 ran 7 seeds x 40 programs over the mock: no deviation"""
    _check(mock_shim, "random", "1", "25")


REF_O1 = os.path.join(ROOT, "oracle", "_ref", "o1")     # the reference's own driver objects (oracle/Makefile `ref`, made by __graft_entry__.build())


def test_reference_driver_over_the_threaded_mock_is_deterministic(tmp_path):
    """the reference's -cycle 0 run at 129^2, 7 levels, V(3,3), over the mock built with OpenMP (as bench.py's CPU baseline builds it), twice
    with different thread counts: rData.dat, uData.dat and eData.dat equal as text.  The mock's dot product -- the reference's first two
    norms go through it -- sums fixed blocks in a fixed order; as an OpenMP reduction it moved rData.dat by an ulp between runs."""
    robjs = [os.path.join(REF_O1, f + ".o") for f in ("array", "matbuild", "mesh", "problem", "solver", "poisson")]
    if not all(os.path.exists(o) for o in robjs):
        pytest.skip("oracle/_ref/o1 is not built (no reference tree at build time)")
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    os.makedirs(OUT, exist_ok=True)
    inc = "-I" + os.path.join(ROOT, "include")
    objs = []
    for cc, std, src, obj in (("g++", "-std=c++17", os.path.join(ROOT, "tests", "mock_mgk.cpp"), "mock_mgk_omp.o"),
                              ("gcc", "-std=c99", os.path.join(ROOT, "multigrid_petsc_amd", "csrc", "petsc_shim.c"), "petsc_shim_omp.o")):
        o = os.path.join(OUT, obj)
        p = subprocess.run([cc, std, "-O1", "-g", "-fopenmp", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L", inc, "-c", src, "-o", o],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    exe = os.path.join(OUT, "refdriver_omp")
    p = subprocess.run(["g++", "-fopenmp", "-o", exe] + robjs + objs + ["-lm", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    opts = ("-npts 129\n-mesh 0\n-iter 1000\n-grids 7\n-levels 7\n-cycle 0\n-map 2\n-v 3,3\n-moreNorm 0\n-pc_type jacobi\n-ksp_richardson_scale 0.8\n")
    text = []
    for run, threads in enumerate(("2", "5")):
        d = tmp_path / str(run)
        d.mkdir()
        (d / "poisson.in").write_text(opts)
        p = subprocess.run([exe], cwd=d, env=dict(os.environ, OMP_NUM_THREADS=threads), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-3000:]
        text.append([(d / name).read_text() for name in ("rData.dat", "uData.dat", "eData.dat")])
    assert len(text[0][0].split()) > 5
    assert text[0] == text[1]


@pytest.mark.parametrize("mode", [None] + list(MODES))
def test_extended_random_programs_under_every_mode_on_the_mock(mock_shim, mode):
    """the extended draw of random_programs_keep_petsc_semantics (2 or 3 levels, uniform or row-table operators, Richardson or Chebyshev
    solvers; 25 programs of up to 60 calls, seed 1) with no switch set and under every mode of shim_semantics.MODES, each in a process of
    its own; the counters of MGPETSC_LAZY_STATS show that the mode's switch switched.  7 seeds x 40 programs in the default mode over the
    mock: the largest error was 0.05 of the tolerance (1e-11 of the magnitude bound)."""
    out = _check(mock_shim, "random", "1", "25", "ext", env=dict(MODES[mode] if mode else {}, MGPETSC_LAZY_STATS="1"))
    random_programs_went_the_way_of_the_mode(mode, lazy_stats(out))
