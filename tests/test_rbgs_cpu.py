"""Red-black Gauss-Seidel, CPU tier.  The reference's own properties (tests/rbgs_reference.py: the colour rule on every level, a sweep at
scale 1 IS Gauss-Seidel, its cycle counts on the issue's table).  The product's mg_solver.c + mg_comm.c + mg_rbgs.c (+ mg_fmg.c, mg_gmres.c,
so that their refusals exist) over host-memory stand-ins for the two kernels, mgk_rbgs_2d_f64 and mgk_prolong_rbgs_2d_f64
(tests/mock_mgk_rbgs.cpp, which includes tests/mock_mgk.cpp textually), driven through Solver(pc_type="rbgs") against the reference: the same
count, the history within 1e-12, u bit for bit; graph=0 and fuse=0 give the bits of the defaults; a second right-hand side on the live handle
and reset + solve; the passes the stand-ins counted; every refusal by its message.  Once more as a plain executable under
-fsanitize=address,undefined.  And the symbols, who names the kernels, and the driver's option."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import rbgs_reference as RB
import rhs_cases
from oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
KERNELS = ("mgk_rbgs_2d_f64", "mgk_prolong_rbgs_2d_f64")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
# (npts, mesh, scale, v0, v1, rhs), levels down to 1 x 1
MOCK_CASES = [(npts, mesh, 1.0, v0, v1, "manufactured") for npts in (17, 33) for mesh in (0, 1) for v0, v1 in ((1, 1), (2, 2), (3, 2), (2, 1))]
SAN_CASES = [(17, 1, 1.0, 3, 2, "manufactured"), (33, 0, 1.0, 2, 2, "manufactured"), (33, 1, 0.8, 2, 1, "manufactured")]
# the reference's cycle counts at rtol 1e-7, manufactured right-hand side, v1 = 3: scale 1 with V(1,1), V(2,2), V(3,3), scale 0.8 with V(2,2).
# 100 is the iteration cap: point relaxation of either kind does not converge within it on the thin cells of -mesh 1 at 513
COUNTS = {(17, 0): (8, 6, 6, 8), (17, 1): (14, 8, 6, 10), (17, 2): (17, 9, 7, 13),
          (65, 0): (8, 6, 6, 8), (65, 1): (34, 16, 11, 23), (65, 2): (22, 11, 8, 17),
          (129, 0): (8, 6, 6, 8), (129, 1): (58, 29, 20, 42), (129, 2): (24, 12, 9, 18),
          (513, 0): (8, 6, 6, 8), (513, 1): (100, 100, 72, 100), (513, 2): (28, 14, 10, 20)}
CONFIGS = ((1.0, 1), (1.0, 2), (1.0, 3), (0.8, 2))


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("npts,mesh", sorted(COUNTS), ids=[f"{n}-mesh{m}" for n, m in sorted(COUNTS)])
def test_reference_counts(orc, npts, mesh):
    got = []
    for scale, v0 in CONFIGS:
        r = RB.reference(orc, (npts, mesh, scale, v0, 3, "manufactured"))
        got.append(r["iters"])
        if r["iters"] < 100:                                # converged: the true residual of the result
            h = RB.hierarchy(orc, npts, mesh)
            n = npts - 2
            res = h.rhs().reshape(n, n) - RB.apply(h.ct[0], r["u"].reshape(n, n))
            assert np.sqrt(np.sum(res * res)) <= RB.RTOL * r["bnorm"] * (1 + 1e-9)
    assert tuple(got) == COUNTS[(npts, mesh)], (npts, mesh, got)


def test_the_colour_rule_on_every_level(orc):
    """on every level of a hierarchy, with that level's own indices: a half-sweep of colour c changes exactly the points with (i + j) & 1 == c
    (random data: every update moves its point) and passes the others through bit for bit; at scale 1 it solves the equations of its
    colour (Gauss-Seidel: the residual vanishes there to rounding); and two half-sweeps are one sweep"""
    rng = np.random.default_rng(11)
    for mesh in (0, 1, 2):
        h = RB.hierarchy(orc, 33, mesh)
        for l in range(h.levels):
            n = h.n[l]
            ct, dinv = h.ct[l], h.dinv[l]
            b, u = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
            i, j = np.indices((n, n))
            for c in (0, 1):
                w = RB.half_sweep(ct, dinv, 1.0, b, u, c)
                mine = ((i + j) & 1) == c
                assert np.array_equal(w[~mine], u[~mine]) and np.all(w[mine] != u[mine]), (mesh, l, c)
                res = b - RB.apply(ct, w)
                assert not mine.any() or np.abs(res[mine]).max() <= 1e-12 * np.abs(ct[:, 2]).max() * max(1.0, np.abs(w).max()), (mesh, l, c)
            one = RB.half_sweep(ct, dinv, 0.8, b, RB.half_sweep(ct, dinv, 0.8, b, u, 0), 1)
            assert np.array_equal(RB.sweeps(ct, dinv, 0.8, b, u, 1), one)
            assert np.array_equal(RB.sweeps(ct, dinv, 0.8, b, None, 2), RB.sweeps(ct, dinv, 0.8, b, np.zeros((n, n)), 2))
    assert RB.colour(3, 4).tolist() == [[0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1]]


def _compile(tag, extra, sources):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src in sources:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"rbgs_{tag}_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + extra + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    return out, objs


def _sources():
    return [os.path.join(HERE, "mock_mgk_rbgs.cpp")] + [os.path.join(CSRC, f) for f in ("mg_solver.c", "mg_comm.c", "mg_rbgs.c", "mg_fmg.c", "mg_gmres.c")]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through Solver in one worker process (the loader caches its libraries); the worker also tries every refusal"""
    out, objs = _compile("plain", [], _sources())
    so = os.path.join(out, "libmgsolve_rbgs_mock.so")
    p = subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    npz = str(tmp_path_factory.mktemp("rbgs") / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "rbgs_mock_worker.py"), so, npz] + [RB.case_key(c) for c in MOCK_CASES],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(npz)


@pytest.mark.parametrize("case", MOCK_CASES, ids=[RB.case_key(c) for c in MOCK_CASES])
def test_rbgs_solve_over_the_mock_equals_the_reference(orc, results, case):
    npts, mesh, scale, v0, v1, rhs = case
    k = RB.case_key(case) + ":"
    ref = RB.reference(orc, case)
    it = int(results[k + "it"])
    RB.compare(ref, it, results[k + "rn"], results[k + "u"], float(results[k + "bnorm"]))
    # per cycle and level: (v0 + 1) / 2 passes down and as many up, the first one up with the prolongation (fuse bit 1); (v1 + 1) / 2 on the
    # coarsest.  From the zero guess: every pre-smoothing but level 0's after the first cycle
    levels, p0, p1 = RB.LEVELS[npts], (v0 + 1) // 2, (v1 + 1) // 2
    plain = it * ((levels - 1) * (2 * p0 - 2) + p1 - 1) + (it - 1)
    zero = it * (levels - 1) + 1
    assert list(results[k + "calls"]) == [plain, zero, it * (levels - 1)], results[k + "calls"]
    n = [(npts - 1) // (1 << l) - 1 for l in range(levels)]
    assert float(results[k + "dof"]) == sum(2 * v0 * m * m for m in n[:-1]) + v1 * n[-1] ** 2          # one sweep: N point updates
    for tag in ("graph0", "fuse0"):
        assert int(results[k + tag + "_it"]) == it
        assert np.array_equal(results[k + tag + "_rn"], results[k + "rn"]) and np.array_equal(results[k + tag + "_u"], results[k + "u"]), tag
    # the second right-hand side on the live handle
    ref2 = RB.reference(orc, (npts, mesh, scale, v0, v1, f"rough:{3}"))
    RB.compare(ref2, int(results[k + "second_it"]), results[k + "second_rn"], results[k + "second_u"], float(results[k + "second_bnorm"]))


@pytest.fixture(scope="module")
def san_exe():
    """the same sources as one executable with -fsanitize=address,undefined, built once"""
    out, objs = _compile("san", SAN, _sources() + [os.path.join(HERE, "san_rbgs.c")])
    exe = os.path.join(out, "san_rbgs")
    p = subprocess.run(["g++"] + SAN + ["-o", exe] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("case", SAN_CASES, ids=[RB.case_key(c) for c in SAN_CASES])
def test_rbgs_solve_under_sanitizers(orc, san_exe, tmp_path, case):
    """under -fsanitize=address,undefined: no report (leaks included: a refused creation leaves nothing), every refusal, a handle that still
    solves after the refused fmg / solve_fmg / solve_gmres, and results that pass the same bars"""
    npts, mesh, scale, v0, v1, rhs = case
    ref = RB.reference(orc, case)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    txt = str(tmp_path / "out.txt")
    p = subprocess.run([san_exe, str(npts), str(RB.LEVELS[npts]), str(mesh), repr(scale), str(v0), str(v1), txt], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:]
    got = {ln.split(" ", 1)[0]: ln.split()[1:] for ln in open(txt)}
    for tag in ("solve", "again", "after"):
        rn = np.array(got[tag + "_rnorm"], dtype=float)
        RB.compare(ref, int(got[tag + "_iters"][0]), rn, np.array(got[tag + "_u"], dtype=float), ref["bnorm"])


def test_the_entry_points_are_built_and_only_mg_rbgs_names_the_kernels():
    """mgk_rbgs_2d_f64 and mgk_prolong_rbgs_2d_f64 are declared and exported by libmgk.so, the hooks by libmgpetsc.so; of the host sources only
    mg_rbgs.c names the kernels (mg_solver.c links against tests/mock_mgk.cpp, which knows neither, in the other host tests)"""
    hk, hs = open(os.path.join(ROOT, "include", "mgk.h")).read(), open(os.path.join(ROOT, "include", "mgsolve.h")).read()
    assert all(k + "(" in hk for k in KERNELS) and "MG_PC_RBGS = 4" in hs
    lib = os.path.join(ROOT, "multigrid_petsc_amd")
    Lk = ctypes.CDLL(os.path.join(lib, "libmgk.so"))
    Lp = ctypes.CDLL(os.path.join(lib, "libmgpetsc.so"))
    assert all(hasattr(Lk, k) for k in KERNELS)
    assert hasattr(Lp, "mg_rbgs_smooth") and hasattr(Lp, "mg_rbgs_prolong_smooth")
    for f in sorted(os.listdir(CSRC)) + [os.path.join("driver", "mgpoisson.c")]:
        if not f.endswith(".c") or f == "mg_rbgs.c":
            continue
        text = open(os.path.join(CSRC, f)).read()
        for name in KERNELS:
            assert name not in text, f"{f} names {name}"
    text = open(os.path.join(CSRC, "mg_rbgs.c")).read()
    assert all(k + "(" in text for k in KERNELS)
    from multigrid_petsc_amd.solver import _PC_GS
    assert _PC_GS == {"rbgs": 4}


def test_a_build_without_mg_rbgs_refuses_the_smoother(tmp_path):
    """mg_solver.c reaches mg_rbgs.c through weak references: linked without it (over the plain stand-in of the kernel ABI, as the other host
    tests link it) creation refuses pc_type rbgs with a message that says so, and every other pc_type value beyond the range by the range check"""
    out, objs = _compile("bare", [], [os.path.join(HERE, "mock_mgk.cpp"), os.path.join(CSRC, "mg_solver.c"), os.path.join(CSRC, "mg_comm.c")])
    src = tmp_path / "bare.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "mgsolve.h"\n'
                   'int main(void) { mg_config c; mg_solver *s = NULL; mg_config_default(&c); c.pc_type = MG_PC_RBGS;\n'
                   '  int rc = mg_solver_create(&s, &c, NULL); printf("%d %s\\n", rc, mg_last_error());\n'
                   '  c.pc_type = 5; rc = mg_solver_create(&s, &c, NULL); printf("%d %s\\n", rc, mg_last_error()); return 0; }\n')
    exe = str(tmp_path / "bare")
    p = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", exe + ".o"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run(["g++", "-o", exe, exe + ".o"] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    lines = p.stdout.strip().split("\n")
    assert p.returncode == 0 and len(lines) == 2, p.stdout
    assert lines[0].startswith("10001 ") and "this build has no red-black Gauss-Seidel smoother" in lines[0], lines[0]
    assert lines[1].startswith("10001 ") and "pc_type must be" in lines[1] and "rbgs (4)" in lines[1], lines[1]


def test_own_driver_takes_pc_type_rbgs(tmp_path):
    """mgpoisson: -pc_type rbgs is accepted; what it does not know stops with exit code 2 and a message that names rbgs and still says
    'only -pc_type jacobi'"""
    exe = os.path.join(ROOT, "multigrid_petsc_amd", "mgpoisson")
    assert os.path.exists(exe), "mgpoisson is not built (csrc/Makefile builds it with the libraries)"
    p = subprocess.run([exe, "-pc_type", "sor"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 2 and "only -pc_type jacobi" in p.stdout and "-pc_type rbgs" in p.stdout, (p.returncode, p.stdout)
    src = open(os.path.join(CSRC, "driver", "mgpoisson.c")).read()
    assert '"rbgs")) c.pc_type = MG_PC_RBGS' in src
