"""V-cycle-preconditioned conjugate gradients, CPU tier.  The product's mg_solver.c + mg_comm.c + mg_cg.c (+ mg_gmres.c) over host-memory
stand-ins for the two fused passes (tests/mock_mgk_cg.cpp, which includes tests/mock_mgk_gmres.cpp textually), driven through Solver.solve_cg()
in one worker process against tests/cg_reference.py: the bars of cg_reference.judge on every case, the call counts of the stand-ins, the
bits of the defaults without the graph and without the fused passes, a second right-hand side, a plain solve afterwards that reproduces a
fresh solver bit for bit, the breakdown case, the refusals, the failed allocation.  Once more as a plain executable under
-fsanitize=address,undefined with leak detection.  And the symbols, who names the kernels, and the driver's option."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cg_reference as R
from oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
RTOL = 1.0e-7
PASSES = ("mgk_cg_direction_apply_dot_f64", "mgk_cg_update_sumsq_f64")
WORKSPACE = ("mgk_cg_workspace_create", "mgk_cg_workspace_destroy", "mgk_cg_workspace_debug")
ALL = R.CASES + [R.BREAKDOWN]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SAN_CASES = [R.CASES[0], R.CASES[5], R.OFF_WIDTH[1]]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


_REF = {}


def _reference(orc, case):
    if case not in _REF:
        _REF[case] = R.reference(orc, case, RTOL)
    return _REF[case]


def _compile(tag, extra, sources):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + HERE]
    objs = []
    for src in sources:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"cg_{tag}_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + extra + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    return out, objs


def _sources():
    return [os.path.join(HERE, "mock_mgk_cg.cpp")] + [os.path.join(CSRC, f) for f in ("mg_solver.c", "mg_comm.c", "mg_cg.c", "mg_gmres.c")]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through Solver in one worker process (the loader caches its libraries)"""
    out, objs = _compile("plain", [], _sources())
    so = os.path.join(out, "libmgsolve_cg_mock.so")
    p = subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    npz = str(tmp_path_factory.mktemp("cg") / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "cg_mock_worker.py"), so, npz] + [R.key(c) for c in ALL],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(npz)


def test_the_case_keys_round_trip():
    assert all(R.parse(R.key(c)) == c for c in ALL) and len({R.key(c) for c in ALL}) == len(ALL)


@pytest.mark.parametrize("case", R.CASES, ids=[R.key(c) for c in R.CASES])
def test_solve_cg_over_the_mock_equals_the_reference(orc, results, case):
    k = R.key(case) + ":"
    it = int(results[k + "it"])
    b, refs = _reference(orc, case)
    R.judge(orc, case, b, refs, it, results[k + "rn"], results[k + "x"], float(results[k + "bnorm"]), RTOL)
    assert int(results[k + "breakdown"]) == 0
    # per solve: `it` launches of each of the two passes; M is applied once before the first step and once after every step but the last
    assert list(results[k + "calls"]) == [it, it, it], results[k + "calls"]
    assert refs[0]["napply"] == it
    assert int(results[k + "it_rhs2"]) >= 1
    # reset + a plain solve after solve_cg: a fresh solver's history and field, bit for bit
    assert int(results[k + "after_it"]) == int(results[k + "plain_it"])
    assert np.array_equal(results[k + "after_rn"], results[k + "plain_rn"]) and np.array_equal(results[k + "after_u"], results[k + "plain_u"])


def test_cg_converges_where_the_plain_iteration_does_not(results):
    """PETSc's default -ksp_richardson_scale 1: the plain iteration has not converged within 100 cycles, CG needs 5 steps (2-D) and 11 (3-D)"""
    for case, steps in ((R.CONVERGED[1], 5), (R.CONVERGED[6], 11)):
        k = R.key(case) + ":"
        assert int(results[k + "it"]) == steps and int(results[k + "plain_it"]) == 100
        assert results[k + "plain_rn"][-1] > RTOL * float(results[k + "bnorm"]) >= results[k + "rn"][-1]


def test_breakdown_with_an_over_relaxed_smoother(orc, results):
    """scale 1.5: M is indefinite, alpha <= 0 in the first step -- in the reference and in the product: no step, the zero field, return code 0"""
    b, refs = _reference(orc, R.BREAKDOWN)
    assert [r["breakdown"] for r in refs] == [1, 1] and [r["iters"] for r in refs] == [0, 0]
    k = R.key(R.BREAKDOWN) + ":"
    assert int(results[k + "it"]) == 0 and int(results[k + "breakdown"]) == 1
    assert not results[k + "x"].any() and len(results[k + "rn"]) == 1 and results[k + "rn"][0] == float(results[k + "bnorm"])
    assert list(results[k + "calls"]) == [1, 0, 1]                  # one cycle, one direction pass, no update
    assert np.array_equal(results[k + "after_u"], results[k + "plain_u"]) and np.array_equal(results[k + "after_rn"], results[k + "plain_rn"])


def test_the_failed_allocation_leaves_a_usable_handle(results):
    assert int(results["alloc_retry_it"]) >= 1


def test_reference_variants_agree_and_converge(orc):
    """the reference itself: both orders of summation give the same count with clear margins, the recurrence residual is the true one, and
    M is symmetric to rounding on every configuration (|a.Mb - b.Ma| <= 3e-14 |a.Mb| on random a, b)"""
    rng = np.random.default_rng(5)
    for case in R.CASES:
        b, refs = _reference(orc, case)
        assert refs[0]["iters"] == refs[1]["iters"] and R.delta(refs[0], refs[1]) <= 1e-13
        for r in refs:
            assert r["breakdown"] == 0
            if not R.capped(case):
                assert abs(r["rnorm"][-1] - r["true"]) <= 1e-5 * r["true"] and r["true"] <= RTOL * r["bnorm"]
        if case[1] <= 67:
            op = R.operators(orc, case)
            x, y = rng.uniform(-1, 1, b.size), rng.uniform(-1, 1, b.size)
            xMy, yMx = float(np.dot(x, op.M(y))), float(np.dot(y, op.M(x)))
            op.close()
            assert abs(xMy - yMx) <= 3e-14 * abs(xMy), (case, xMy, yMx)


@pytest.fixture(scope="module")
def san_exe():
    """the same sources as one executable with -fsanitize=address,undefined, built once"""
    out, objs = _compile("san", SAN, _sources() + [os.path.join(HERE, "san_cg.c")])
    exe = os.path.join(out, "san_cg")
    p = subprocess.run(["g++"] + SAN + ["-o", exe] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("case", SAN_CASES, ids=[R.key(c) for c in SAN_CASES])
def test_solve_cg_under_sanitizers(orc, san_exe, tmp_path, case):
    """a stand-alone executable under -fsanitize=address,undefined: no report (leaks included: the failed allocation frees what it had, and
    mg_solver_destroy frees the fields and the workspace), the refusals, and results that pass the same bars"""
    dim, npts, levels, scale, v, rhs, maxiter = case
    b, refs = _reference(orc, case)
    rhsfile = "-"
    if rhs != "manufactured":
        rhsfile = str(tmp_path / "rhs.bin")
        b.tofile(rhsfile)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    txt = str(tmp_path / "out.txt")
    p = subprocess.run([san_exe, str(dim), str(npts), str(levels), repr(scale), str(v[0]), str(v[1]), str(maxiter), rhsfile, txt], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:]
    got = {ln.split(" ", 1)[0]: ln.split()[1:] for ln in open(txt)}
    rn = np.array(got["cg_rnorm"], dtype=float)
    R.judge(orc, case, b, refs, int(got["cg_iters"][0]), rn, np.array(got["cg_u"], dtype=float), rn[0], RTOL)
    assert int(got["cg_breakdown"][0]) == 0
    plain = orc.vcycle(dim, npts, levels, v[0], v[1], maxiter=maxiter, scale=scale, b=None if rhs == "manufactured" else b)
    assert int(got["after_iters"][0]) == plain["iters"]
    assert np.array_equal(np.array(got["after_u"], dtype=float), plain["u"])


def test_the_cg_entry_points_are_built_and_only_mg_cg_names_the_kernels():
    """the passes and their workspace are declared by include/mgk_cg.h (not include/mgk.h) and exported by libmgk.so, mg_solver_solve_cg and
    mg_solver_cg_breakdown by libmgpetsc.so; of the host sources only mg_cg.c names them, and mg_solver.c names nothing of mg_cg.c"""
    hc, hk, hs = (open(os.path.join(ROOT, "include", f)).read() for f in ("mgk_cg.h", "mgk.h", "mgsolve.h"))
    assert all(k + "(" in hc and k not in hk for k in PASSES + WORKSPACE)
    assert "mg_solver_solve_cg(" in hs and "mg_solver_cg_breakdown(" in hs
    lib = os.path.join(ROOT, "multigrid_petsc_amd")
    Lk = ctypes.CDLL(os.path.join(lib, "libmgk.so"))
    Lp = ctypes.CDLL(os.path.join(lib, "libmgpetsc.so"))
    assert all(hasattr(Lk, k) for k in PASSES + WORKSPACE)
    assert hasattr(Lp, "mg_solver_solve_cg") and hasattr(Lp, "mg_solver_cg_breakdown")
    for f in ("mg_solver.c", "mg_comm.c", "mg_fmg.c", "mg_cheby.c", "mg_gmres.c", "petsc_shim.c", os.path.join("driver", "mgpoisson.c")):
        text = open(os.path.join(CSRC, f)).read()
        for name in PASSES + WORKSPACE:
            assert name not in text, f"{f} names {name}"
    for f in ("mg_solver.c", "mg_fmg.c", "mg_cheby.c", "petsc_shim.c", os.path.join("driver", "mgpoisson.c")):
        assert "mgk_multi_dot_f64" not in open(os.path.join(CSRC, f)).read(), f
    solver = open(os.path.join(CSRC, "mg_solver.c")).read()
    assert "mg_solver_solve_cg" not in solver and "mg_solver_cg_breakdown" not in solver and "mgk_cg" not in solver
    text = open(os.path.join(CSRC, "mg_cg.c")).read()
    assert all(k + "(" in text for k in PASSES) and "mgk_multi_dot_f64(" in text
    # the two kernels keep away from the context's shared reduction scratch
    unit = open(os.path.join(CSRC, "mgk_cg.hip")).read()
    assert "->partials" not in unit and ".partials" not in unit


def test_own_driver_checks_the_krylov_option_before_it_touches_the_gpu(tmp_path):
    """mgpoisson: -mg_krylov takes cg or none and excludes -mg_accel gmres; anything else stops with exit code 2 and a message"""
    exe = os.path.join(ROOT, "multigrid_petsc_amd", "mgpoisson")
    if not os.path.exists(exe):
        pytest.skip("mgpoisson is not built")
    for args, msg in ((["-mg_krylov", "gmres"], "-mg_krylov must be"), (["-mg_krylov", "cg", "-mg_accel", "gmres"], "exclude each other")):
        p = subprocess.run([exe] + args, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert p.returncode == 2 and msg in p.stdout, (args, p.returncode, p.stdout)


def test_a_driver_built_without_mg_cg_links_and_refuses_the_option(tmp_path):
    """mgpoisson.c + mg_solver.c + mg_comm.c over tests/mock_mgk.cpp alone (no mg_cg.c, no mg_gmres.c): links, runs a plain solve, and
    refuses -mg_krylov cg with exit code 2; linked with mg_cg.c over the CG stand-ins it prints the reference's step count"""
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    flags = ["-O1", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + HERE]
    host = [os.path.join(CSRC, "driver", "mgpoisson.c"), os.path.join(CSRC, "mg_solver.c"), os.path.join(CSRC, "mg_comm.c")]
    common = ["-dim", "2", "-npts", "65", "-levels", "5", "-iter", "100", "-ksp_richardson_scale", "1.0", "-pc_type", "jacobi", "-write_fields", "0"]
    for mock, extra, want in (("mock_mgk.cpp", [], None), ("mock_mgk_cg.cpp", [os.path.join(CSRC, "mg_cg.c"), os.path.join(CSRC, "mg_gmres.c")], 5)):
        o = str(tmp_path / (mock + ".o"))
        exe = str(tmp_path / ("mgpoisson_" + mock[:-4]))
        for cmd in (["g++", "-std=c++17"] + flags + ["-c", os.path.join(HERE, mock), "-o", o],
                    ["gcc", "-std=c99"] + flags + host + extra + [o, "-o", exe, "-lstdc++", "-lm", "-ldl", "-lpthread"]):
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert p.returncode == 0, p.stdout[-3000:]
        p = subprocess.run([exe] + common + ["-mg_krylov", "cg"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        if want is None:
            assert p.returncode == 2 and "this build has no CG" in p.stdout, p.stdout[-2000:]
        else:
            assert p.returncode == 0 and f"Number of iterations:\t\t{want}" in p.stdout, p.stdout[-2000:]
