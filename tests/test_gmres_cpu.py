"""V-cycle-preconditioned GMRES, CPU tier.  The product's mg_solver.c + mg_comm.c + mg_gmres.c over host-memory stand-ins for the Krylov entry
points (tests/mock_mgk_gmres.cpp, which includes tests/mock_mgk.cpp textually), driven through Solver against tests/gmres_reference.py:
the same count, x and the history within 100 delta of the reference (delta = the distance between the reference's two orders of summation,
floor 1e-13: the bound of tests/test_gmres_solve_gpu.py), a converged true residual, fewer applications of the cycle than V-cycles; a plain
solve afterwards reproduces a fresh solver bit for bit; the stand-ins' call counts show one multi-dot, one multi-axpy and ONE fetch per step.
Once more as a plain executable under -fsanitize=address,undefined, with the refusals.  And the symbols, and who names the kernels."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gmres_reference as G
import rhs_cases
from oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
RTOL = 1.0e-7
KERNELS = ("mgk_multi_dot_f64", "mgk_multi_axpy_sumsq_f64", "mgk_krylov_fetch", "mgk_lincomb_f64", "mgk_scale_to_f64")
# (dim, npts, levels, mesh, scale, restart, rhs, maxiter): the small cases of tests/test_gmres_solve_gpu.py
CASES = [
    (2, 65, 5, 0, 0.8, 30, "manufactured", 100),
    (2, 65, 5, 1, 0.8, 30, "manufactured", 100),
    (2, 65, 5, 1, 0.8, 5, "rough:12", 100),
    (2, 65, 5, 2, 0.8, 30, "manufactured", 100),
    (3, 33, 4, 0, 0.8, 30, "rough:3", 100),
    (3, 33, 4, 0, 1.0, 4, "manufactured", 100),
]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _key(case):
    return ",".join(str(c) for c in case)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


_REF = {}


def _reference(orc, case):
    if case not in _REF:
        dim, npts, levels, mesh, scale, restart, rhs, maxiter = case
        op = G.Operators(orc, dim, npts, levels, mesh, scale)
        b = op.rhs() if rhs == "manufactured" else rhs_cases.uniform(dim, npts, int(rhs.split(":")[1]))
        refs = [G.gmres(op, b, restart, rtol=RTOL, maxiter=maxiter, dot=d) for d in ("np", "ld")]
        op.close()
        _REF[case] = (b, refs)
    return _REF[case]


def _compile(tag, extra, sources):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src in sources:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"gmres_{tag}_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + extra + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    return out, objs


def _sources():
    return [os.path.join(HERE, "mock_mgk_gmres.cpp"), os.path.join(CSRC, "mg_solver.c"), os.path.join(CSRC, "mg_comm.c"), os.path.join(CSRC, "mg_gmres.c")]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through Solver in one worker process (the loader caches its libraries)"""
    out, objs = _compile("plain", [], _sources())
    so = os.path.join(out, "libmgsolve_gmres_mock.so")
    p = subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    npz = str(tmp_path_factory.mktemp("gmres") / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "gmres_mock_worker.py"), so, npz] + [_key(c) for c in CASES],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(npz)


def _compare(orc, case, it, rn, x, bnorm):
    """the bars of the GPU tier on a result of the product's host code"""
    dim, npts, levels, mesh, scale, restart, rhs, maxiter = case
    b, refs = _reference(orc, case)
    G.judge(orc, (dim, npts, levels, mesh, scale), b, refs, it, rn, x, bnorm, RTOL)      # (the bars themselves: shared with the session draw)
    return refs


@pytest.mark.parametrize("case", CASES, ids=[_key(c) for c in CASES])
def test_solve_gmres_over_the_mock_equals_the_reference(orc, results, case):
    k = _key(case) + ":"
    it, restart = int(results[k + "it"]), case[5]
    refs = _compare(orc, case, it, results[k + "rn"], results[k + "x"], float(results[k + "bnorm"]))
    # one multi-dot, one multi-axpy and ONE fetch (the step's only synchronisation) per step; one lincomb per correction; v_0 of every
    # restart cycle and every v_{j+1} that is used come from scale_to
    ncorr = -(-it // restart)
    assert list(results[k + "calls"]) == [it, it, it, ncorr, it], results[k + "calls"]
    assert refs[0]["napply"] == it + ncorr
    assert int(results[k + "it_other_restart"]) >= 1
    # a plain solve after solve_gmres: a fresh solver's history and field, bit for bit
    assert int(results[k + "after_it"]) == int(results[k + "plain_it"])
    assert np.array_equal(results[k + "after_rn"], results[k + "plain_rn"]) and np.array_equal(results[k + "after_u"], results[k + "plain_u"])


def test_gmres_accelerates(orc, results):
    """fewer applications of the cycle than V-cycles on both stretched meshes; at Richardson scale 1 it converges within 10 steps where
    the cycle alone has not within 100"""
    for case in (CASES[1], CASES[3]):
        k = _key(case) + ":"
        it = int(results[k + "it"])
        assert it + -(-it // case[5]) < int(results[k + "plain_it"]), (case, it, int(results[k + "plain_it"]))
    k = _key(CASES[5]) + ":"
    assert int(results[k + "it"]) <= 10 and int(results[k + "plain_it"]) == 100
    assert results[k + "plain_rn"][-1] > RTOL * float(results[k + "bnorm"]) >= results[k + "rn"][-1]


@pytest.fixture(scope="module")
def san_exe():
    """the same sources as one executable with -fsanitize=address,undefined, built once"""
    out, objs = _compile("san", SAN, _sources() + [os.path.join(HERE, "san_gmres.c")])
    exe = os.path.join(out, "san_gmres")
    p = subprocess.run(["g++"] + SAN + ["-o", exe] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3], CASES[5]], ids=[_key(c) for c in (CASES[0], CASES[2], CASES[3], CASES[5])])
def test_solve_gmres_under_sanitizers(orc, san_exe, tmp_path, case):
    """under -fsanitize=address,undefined: no report (leaks included: the basis is freed at a new restart length and by
    mg_solver_destroy), the refusals, and results that pass the same bars"""
    dim, npts, levels, mesh, scale, restart, rhs, maxiter = case
    exe = san_exe
    b, refs = _reference(orc, case)
    rhsfile = "-"
    if rhs != "manufactured":
        rhsfile = str(tmp_path / "rhs.bin")
        b.tofile(rhsfile)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    txt = str(tmp_path / "out.txt")
    p = subprocess.run([exe, str(dim), str(npts), str(levels), str(mesh), repr(scale), str(restart), str(maxiter), rhsfile, txt], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:]
    got = {ln.split(" ", 1)[0]: ln.split()[1:] for ln in open(txt)}
    rn = np.array(got["gmres_rnorm"], dtype=float)
    _compare(orc, case, int(got["gmres_iters"][0]), rn, np.array(got["gmres_u"], dtype=float), rn[0])
    plain = orc.vcycle(dim, npts, levels, 3, 3, maxiter=maxiter, scale=scale, use_csr=1 if mesh else 0, mesh=mesh, b=None if rhs == "manufactured" else b)
    assert int(got["after_iters"][0]) == plain["iters"]
    assert np.array_equal(np.array(got["after_u"], dtype=float), plain["u"])


def test_reference_variants_agree_and_converge(orc):
    """the reference itself: both orders of summation give the same count with clear margins, and the estimate is the true residual"""
    for case in CASES:
        b, refs = _reference(orc, case)
        assert refs[0]["iters"] == refs[1]["iters"]
        assert G.delta(refs[0], refs[1]) <= 1e-13
        for r in refs:
            assert abs(r["rnorm"][-1] - r["true"]) <= 1e-6 * r["true"]
            assert r["true"] <= RTOL * r["bnorm"]


def test_the_gmres_entry_points_are_built_and_only_mg_gmres_names_the_kernels():
    """the five kernels are declared and exported by libmgk.so, mg_solver_solve_gmres by libmgpetsc.so; of the host sources only mg_gmres.c
    names the kernels (mg_solver.c links against tests/mock_mgk.cpp, which knows none of them, in the other host tests)"""
    hk, hs = open(os.path.join(ROOT, "include", "mgk.h")).read(), open(os.path.join(ROOT, "include", "mgsolve.h")).read()
    assert all(k + "(" in hk for k in KERNELS) and "mg_solver_solve_gmres(" in hs and "#define MGK_KRYLOV_MAX 33" in hk
    lib = os.path.join(ROOT, "multigrid_petsc_amd")
    Lk = ctypes.CDLL(os.path.join(lib, "libmgk.so"))
    Lp = ctypes.CDLL(os.path.join(lib, "libmgpetsc.so"))
    assert all(hasattr(Lk, k) for k in KERNELS)
    assert hasattr(Lp, "mg_solver_solve_gmres") and hasattr(Lp, "mgi_apply_cycle")
    for f in ("mg_solver.c", "mg_comm.c", "mg_fmg.c", "mg_cheby.c", "petsc_shim.c", os.path.join("driver", "mgpoisson.c")):
        text = open(os.path.join(CSRC, f)).read()
        for name in KERNELS:
            assert name not in text, f"{f} names {name}"
    assert "mg_solver_solve_gmres" not in open(os.path.join(CSRC, "mg_solver.c")).read()
    text = open(os.path.join(CSRC, "mg_gmres.c")).read()
    assert all(k + "(" in text for k in KERNELS)


def test_own_driver_checks_the_gmres_options_before_it_touches_the_gpu(tmp_path):
    """mgpoisson: -mg_accel takes gmres or none, -mg_gmres_restart 1 .. 32; anything else stops with exit code 2 and a message"""
    exe = os.path.join(ROOT, "multigrid_petsc_amd", "mgpoisson")
    if not os.path.exists(exe):
        pytest.skip("mgpoisson is not built")
    for args, msg in ((["-mg_accel", "cg"], "-mg_accel must be"), (["-mg_accel", "gmres", "-mg_gmres_restart", "33"], "-mg_gmres_restart must be within"),
                      (["-mg_accel", "gmres", "-mg_gmres_restart", "0"], "-mg_gmres_restart must be within")):
        p = subprocess.run([exe] + args, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert p.returncode == 2 and msg in p.stdout, (args, p.returncode, p.stdout)
