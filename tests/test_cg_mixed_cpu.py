"""Conjugate gradients over the fp32 cycle of the mixed-precision solver, CPU tier.  The product's mg_solver.c + mg_comm.c + mg_cg.c + mg_cg_mixed.c
(+ mg_gmres.c) over host-memory stand-ins for the three passes (tests/mock_mgk_cg_mixed.cpp, which includes tests/mock_mgk_cg.cpp textually),
driven through Solver.solve_cg_mixed() in one worker process against tests/cg_mixed_reference.py: the bars of cg_reference.judge on every case,
the call counts of the stand-ins, a second right-hand side, a plain mixed solve afterwards that reproduces a fresh solver bit for bit, the
breakdown case, the refusals, the failed allocation, and the scale-1 case that the plain mixed iteration does not converge on.  Once more as a
plain executable under -fsanitize=address,undefined with leak detection.  And the reference's own properties, the symbols, and the driver's option."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cg_mixed_reference as R
from oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
RTOL = 1.0e-7
PASSES = ("mgk_cg_dot_f64_f32", "mgk_cg_direction_apply_dot_zf32_f64", "mgk_cg_update_sumsq_f64_f32")
ALL = R.CASES + [R.BREAKDOWN, R.SCALE_ONE]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SAN_CASES = [R.CONVERGED[0], R.OFF_WIDTH[0]]
# what the reference gives on the CPU (steps, last and previous entry in units of rtol ||b||), as the issue of this entry point records it
RECORDED = {R.CONVERGED[0]: (7, 0.19, 3.20), R.CONVERGED[1]: (7, 0.19, 2.80), R.OFF_WIDTH[0]: (15, 0.56, 2.58)}
HOST = ("mg_solver.c", "mg_comm.c", "mg_cg.c", "mg_cg_mixed.c", "mg_gmres.c")


@pytest.fixture(scope="module")
def orc():
    return Oracle()


_REF = {}


def _reference(orc, case):
    if case not in _REF:
        _REF[case] = R.reference(orc, case, RTOL)
    return _REF[case]


def _need_compilers():
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")


def _compile(tag, extra, sources):
    _need_compilers()
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + HERE]
    objs = []
    for src in sources:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"cgm_{tag}_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + extra + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    return out, objs


def _sources():
    return [os.path.join(HERE, "mock_mgk_cg_mixed.cpp")] + [os.path.join(CSRC, f) for f in HOST]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through Solver in one worker process (the loader caches its libraries)"""
    out, objs = _compile("plain", [], _sources())
    so = os.path.join(out, "libmgsolve_cg_mixed_mock.so")
    p = subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    npz = str(tmp_path_factory.mktemp("cgm") / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "cg_mixed_mock_worker.py"), so, npz] + [R.key(c) for c in ALL],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(npz)


def test_the_case_keys_round_trip():
    assert all(R.parse(R.key(c)) == c for c in ALL) and len({R.key(c) for c in ALL}) == len(ALL)
    assert all(R.capped(c) for c in R.CAPPED) and not any(R.capped(c) for c in R.CONVERGED + R.OFF_WIDTH + [R.SCALE_ONE])


def test_the_reference_has_the_recorded_counts_margins_residual_and_symmetry(orc):
    """the reference itself: equal counts in both orders of summation with the recorded margins, the recurrence residual within 1e-5 of the
    true one, and the mixed M symmetric to 1e-6 (3e-7 measured) -- fp32 rounding, where the fp64 cycle is symmetric to 3e-14"""
    for case in R.CONVERGED + R.OFF_WIDTH:
        b, refs = _reference(orc, case)
        steps, last, before = RECORDED[case]
        assert refs[0]["iters"] == refs[1]["iters"] == steps
        for r in refs:
            got = R.margins(r, RTOL)
            assert r["breakdown"] == 0 and abs(got[0] - last) <= 0.01 and abs(got[1] - before) <= 0.01, (case, got)
            assert abs(r["rnorm"][-1] - r["true"]) <= 1e-5 * r["true"] and r["true"] <= RTOL * r["bnorm"]
        print(f"\n{R.key(case)}: steps {steps}, margins {R.margins(refs[0], RTOL)}, delta {R.delta(refs[0], refs[1]):.2e}")
    for case, to_tol in zip(R.CAPPED, (30, 19)):
        b, refs = _reference(orc, case)
        assert refs[0]["iters"] == refs[1]["iters"] == case[6] < to_tol and refs[0]["breakdown"] == refs[1]["breakdown"] == 0
    for case in (R.CONVERGED[0], R.CAPPED[1], R.OFF_WIDTH[0]):
        a = R.asymmetry(orc, case)
        print(f"asymmetry of the mixed M on {R.key(case)}: {a:.2e}")
        assert a <= 1e-6, (case, a)


@pytest.mark.parametrize("case", R.CASES, ids=[R.key(c) for c in R.CASES])
def test_solve_cg_mixed_over_the_mock_equals_the_reference(orc, results, case):
    k = R.key(case) + ":"
    it = int(results[k + "it"])
    b, refs = _reference(orc, case)
    R.judge(orc, case, b, refs, it, results[k + "rn"], results[k + "x"], float(results[k + "bnorm"]), RTOL)
    assert int(results[k + "breakdown"]) == 0
    # per solve: `it` launches of each of the three passes (M is applied once before the first step and once after every step but the last,
    # and every application is followed by the dot); none of the fp64 passes, no mgk_multi_dot_f64
    assert list(results[k + "calls"]) == [it, it, it, 0, 0, 0], results[k + "calls"]
    assert refs[0]["napply"] == it
    assert int(results[k + "it_rhs2"]) >= 1
    # reset + a plain mixed solve after solve_cg_mixed: a fresh mixed solver's history and field, bit for bit
    assert int(results[k + "after_it"]) == int(results[k + "plain_it"])
    assert np.array_equal(results[k + "after_rn"], results[k + "plain_rn"]) and np.array_equal(results[k + "after_u"], results[k + "plain_u"])


def test_cg_converges_at_scale_one_where_the_plain_mixed_iteration_does_not(orc, results):
    """PETSc's default -ksp_richardson_scale 1 at 33^3: the plain mixed iteration has not converged within 100 cycles; CG over the same fp32 cycle
    takes the reference's 30 steps to a converged TRUE residual (the stop margin of that case is not clear of rounding, so the count is held to the
    reference's two orders, which agree, and the solution to the true residual, not to judge's bars)"""
    case = R.SCALE_ONE
    b, refs = _reference(orc, case)
    assert refs[0]["iters"] == refs[1]["iters"] == 30
    k = R.key(case) + ":"
    bnorm = float(results[k + "bnorm"])
    assert int(results[k + "plain_it"]) == 100 and results[k + "plain_rn"][-1] > RTOL * bnorm
    assert int(results[k + "it"]) == 30 and int(results[k + "breakdown"]) == 0 and results[k + "rn"][-1] <= RTOL * bnorm
    op = R.MixedOperators(orc, case)
    r = b - op.A(results[k + "x"])
    op.close()
    assert np.sqrt(np.dot(r, r)) <= RTOL * bnorm * (1.0 + 1e-3)


def test_breakdown_with_an_over_relaxed_smoother(orc, results):
    """scale 1.5: M is indefinite, beta < 0 after the first completed update -- what the reference reports in both orders is what the product
    reports: the step, the count, one entry of history beyond ||b||, the x of that step, return code 0"""
    b, refs = _reference(orc, R.BREAKDOWN)
    assert refs[0]["breakdown"] == refs[1]["breakdown"] >= 1 and refs[0]["iters"] == refs[1]["iters"]
    k = R.key(R.BREAKDOWN) + ":"
    it = int(results[k + "it"])
    assert it == refs[0]["iters"] and int(results[k + "breakdown"]) == refs[0]["breakdown"]
    assert len(results[k + "rn"]) == it + 1 and results[k + "rn"][0] == float(results[k + "bnorm"])
    bound = max(100.0 * R.delta(refs[0], refs[1]), 1e-13)
    assert min(R.distance(results[k + "x"], results[k + "rn"], r) for r in refs) <= bound
    napply = refs[0]["napply"]
    assert list(results[k + "calls"]) == [napply, refs[0]["breakdown"], it, 0, 0, 0], results[k + "calls"]
    assert np.array_equal(results[k + "after_u"], results[k + "plain_u"]) and np.array_equal(results[k + "after_rn"], results[k + "plain_rn"])


def test_the_failed_allocation_leaves_a_usable_handle(results):
    assert int(results["alloc_retry_it"]) >= 1


@pytest.fixture(scope="module")
def san_exe():
    """the same sources as one executable with -fsanitize=address,undefined, built once"""
    out, objs = _compile("san", SAN, _sources() + [os.path.join(HERE, "san_cg_mixed.c")])
    exe = os.path.join(out, "san_cg_mixed")
    p = subprocess.run(["g++"] + SAN + ["-o", exe] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("case", SAN_CASES, ids=[R.key(c) for c in SAN_CASES])
def test_solve_cg_mixed_under_sanitizers(orc, san_exe, tmp_path, case):
    """a stand-alone executable under -fsanitize=address,undefined: no report (leaks included), every refusal, and results that pass the same bars"""
    dim, npts, levels, scale, v, rhs, maxiter = case
    b, refs = _reference(orc, case)
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
    plain = orc.vcycle_mixed(npts, levels, v[0], v[1], maxiter=maxiter, scale=scale, b=b)
    assert int(got["after_iters"][0]) == plain["iters"]
    assert np.array_equal(np.array(got["after_u"], dtype=float), plain["u"])


def test_the_entry_points_are_built_and_only_mg_cg_mixed_names_the_kernels():
    """the three passes are declared by include/mgk_cg_mixed.h (not by mgk.h or mgk_cg.h) and exported by libmgk.so, mg_solver_solve_cg_mixed by
    libmgpetsc.so; of the host sources only mg_cg_mixed.c names them, and only the driver (weakly) and that file name the entry point"""
    hm, hc, hk, hs = (open(os.path.join(ROOT, "include", f)).read() for f in ("mgk_cg_mixed.h", "mgk_cg.h", "mgk.h", "mgsolve.h"))
    assert all(k + "(" in hm and k not in hk and k not in hc for k in PASSES)
    assert "mg_solver_solve_cg_mixed(" in hs
    lib = os.path.join(ROOT, "multigrid_petsc_amd")
    Lk = ctypes.CDLL(os.path.join(lib, "libmgk.so"))
    Lp = ctypes.CDLL(os.path.join(lib, "libmgpetsc.so"))
    assert all(hasattr(Lk, k) for k in PASSES) and hasattr(Lp, "mg_solver_solve_cg_mixed")
    for f in sorted(os.listdir(CSRC)) + [os.path.join("driver", "mgpoisson.c")]:
        if not f.endswith(".c") or f == "mg_cg_mixed.c":
            continue
        text = open(os.path.join(CSRC, f)).read()
        for name in PASSES:
            assert name not in text, f"{f} names {name}"
        if f != os.path.join("driver", "mgpoisson.c") and f != "mg_cg.c":          # (mg_cg.c: in the message of its refusal)
            assert "mg_solver_solve_cg_mixed" not in text, f
    assert "mg_solver_solve_cg_mixed(mg_solver *s) __attribute__((weak))" in open(os.path.join(CSRC, "driver", "mgpoisson.c")).read()
    text = open(os.path.join(CSRC, "mg_cg_mixed.c")).read()
    assert all(k + "(" in text for k in PASSES)
    unit = open(os.path.join(CSRC, "mgk_cg_mixed.hip")).read() + open(os.path.join(CSRC, "mgk_cg_dev.hpp")).read()
    assert "->partials" not in unit and ".partials" not in unit              # the context's shared reduction scratch is not used


def test_own_driver_with_and_without_mg_cg_mixed(orc, tmp_path):
    """mgpoisson.c over the stand-ins: linked with mg_cg_mixed.c, -mg_krylov cg -precision mixed prints the reference's step count for the
    manufactured right-hand side; linked without it (mg_cg.c alone) the combination is refused with exit code 2 and fp64 CG still runs"""
    _need_compilers()
    flags = ["-O1", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + HERE]
    host = [os.path.join(CSRC, f) for f in (os.path.join("driver", "mgpoisson.c"), "mg_solver.c", "mg_comm.c", "mg_cg.c", "mg_gmres.c")]
    case = (3, 17, 3, 0.8, (3, 3), "manufactured", 100)
    op = R.MixedOperators(orc, case)
    want = R.cg(op, op.rhs(), rtol=RTOL, maxiter=100)
    op.close()
    assert want["breakdown"] == 0 and R.margins(want, RTOL)[0] <= 0.8 <= 1.5 <= R.margins(want, RTOL)[1]
    common = ["-dim", "3", "-npts", "17", "-levels", "3", "-iter", "100", "-ksp_richardson_scale", "0.8", "-pc_type", "jacobi", "-write_fields", "0"]
    o = str(tmp_path / "mock.o")
    p = subprocess.run(["g++", "-std=c++17"] + flags + ["-c", os.path.join(HERE, "mock_mgk_cg_mixed.cpp"), "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    for tag, extra in (("with", [os.path.join(CSRC, "mg_cg_mixed.c")]), ("without", [])):
        exe = str(tmp_path / ("mgpoisson_" + tag))
        p = subprocess.run(["gcc", "-std=c99"] + flags + host + extra + [o, "-o", exe, "-lstdc++", "-lm", "-ldl", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        p = subprocess.run([exe] + common + ["-mg_krylov", "cg", "-precision", "mixed"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        if tag == "with":
            assert p.returncode == 0 and f"Number of iterations:\t\t{want['iters']}" in p.stdout, p.stdout[-2000:]
        else:
            assert p.returncode == 2 and "this build has no mixed-precision CG" in p.stdout, p.stdout[-2000:]
            p = subprocess.run([exe] + common + ["-mg_krylov", "cg"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            assert p.returncode == 0 and "Number of iterations:" in p.stdout, p.stdout[-2000:]
