"""KSPCHEBYSHEV on the fused cycle (fuse bit 15), CPU tier.  The product's mg_solver.c + mg_comm.c + mg_cheby.c over host-memory stand-ins
for the five Chebyshev entry points (tests/mock_mgk_cheby.cpp, which includes tests/mock_mgk.cpp textually), driven through Solver against
the CPU oracle: same iteration count, bit-identical solution, over a solve and over a fixed run of cycles with the coarse-level graph
recorded and replayed; the stand-ins count their executions, which shows that the fused path really runs (and does not with bit 15 off).
Once more as a plain executable under -fsanitize=address,undefined.  And, on the oracle alone, the motive: Chebyshev needs fewer cycles."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
EIG = (0.2, 2.0)
NCYC = 5
KERNELS = ("mgk_cheby3_2d_f64", "mgk_cheby3_2d_sumsq_f64", "mgk_cheby3_2d_zero_f64", "mgk_prolong_cheby3_2d_f64", "mgk_tail_cycle_cheby_f64")
# (dim, npts, levels, mesh): full depth.  2-D 33 / 129: every level below the finest is in the tail; 257: level 1 (127^2) is launched
CASES = [(2, 33, 5, 0), (2, 129, 7, 0), (2, 257, 8, 0), (2, 129, 7, 1), (2, 129, 7, 2), (3, 33, 5, 0)]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _compile(tag, extra, sources):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src in sources:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"cheby_{tag}_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + extra + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    return out, objs


def _sources():
    return [os.path.join(HERE, "mock_mgk_cheby.cpp"), os.path.join(CSRC, "mg_solver.c"), os.path.join(CSRC, "mg_comm.c"), os.path.join(CSRC, "mg_cheby.c")]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through Solver in one worker process (the loader caches its libraries), default mask and bit 15 off"""
    out, objs = _compile("plain", [], _sources())
    so = os.path.join(out, "libmgsolve_cheby_mock.so")
    p = subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    npz = str(tmp_path_factory.mktemp("cheby") / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "cheby_mock_worker.py"), so, npz] + [",".join(map(str, c)) for c in CASES],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(npz)


def _oracle(orc, dim, npts, levels, mesh, fixed=0):
    return orc.vcycle(dim, npts, levels, 3, 3, maxiter=60, ksp_type=1, emin=EIG[0], emax=EIG[1], use_csr=1 if mesh else 0, fixed_cycles=fixed, mesh=mesh)


def _ltail(dim, npts, levels):
    """first level inside the tail kernel (n <= 63 in 2-D, <= 15 in 3-D), as mg_solver_create chooses it"""
    for l in range(1, levels):
        if (npts - 1) // 2 ** l - 1 <= (15 if dim == 3 else 63):
            return l if 2 <= levels - l <= 8 else 0
    return 0


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("dim,npts,levels,mesh", CASES)
def test_fused_chebyshev_cycle_equals_the_oracle(orc, results, dim, npts, levels, mesh):
    k = f"{dim},{npts},{levels},{mesh}:"
    ref = _oracle(orc, dim, npts, levels, mesh)
    ref5 = _oracle(orc, dim, npts, levels, mesh, fixed=NCYC)
    for tag in ("on", "off"):
        it, rn, u = int(results[k + tag + ":it"]), results[k + tag + ":rn"], results[k + tag + ":u"]
        assert it == ref["iters"], (tag, it, ref["iters"])
        assert np.abs(rn / ref["rnorm"] - 1).max() <= 1e-12, tag
        assert np.array_equal(u, ref["u"]), tag          # (-mesh 1/2: the oracle's assembled leg, as the existing mesh tests)
        rn5, u5 = results[k + tag + ":rn5"], results[k + tag + ":u5"]
        assert len(rn5) == NCYC + 1 and np.abs(rn5 / ref5["rnorm"] - 1).max() <= 1e-12, tag
        assert np.array_equal(u5, ref5["u"]), tag
    # the default mask and bit 15 off: the same bits, over the solve and over the fixed run (graph recorded in cycle 1, replayed after)
    for f in ("u", "u5", "rn", "rn5"):
        assert np.array_equal(results[k + "on:" + f], results[k + "off:" + f]), f


@pytest.mark.parametrize("dim,npts,levels,mesh", CASES)
def test_the_fused_passes_really_run(results, dim, npts, levels, mesh):
    """executions of the stand-ins: per cycle two three-step passes on every 2-D level above the tail (pre- and post-smoothing; on level 0
    the norm pass of the cycle before and the prolongation pass) and one tail call; the solve may end with one speculative norm pass
    outstanding; a fixed run knows its last cycle and makes none.  With bit 15 off: none of either"""
    k = f"{dim},{npts},{levels},{mesh}:"
    lt = _ltail(dim, npts, levels)
    assert lt >= 1
    above = lt if dim == 2 else 0
    it = int(results[k + "on:it"])
    c, c5 = results[k + "on:calls"], results[k + "on:calls5"]
    assert c[4] == it and c5[4] == NCYC
    assert c[:4].sum() in (2 * above * it, 2 * above * it + 1), (c, it)
    assert c5[:4].sum() == 2 * above * NCYC, c5
    if dim == 2:
        assert c5[3] == above * NCYC                                   # one prolongation pass per level and cycle
        assert c5[2] >= (above - 1) * NCYC + 1                          # zero-guess passes: the inner levels, and level 0 in the first cycle
        assert c5[1] >= 1                                               # the norm pass of a cycle makes the next one's pre-smoothing
    assert not results[k + "off:calls"].any() and not results[k + "off:calls5"].any()


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("dim,npts,levels,mesh", [(2, 33, 5, 0), (2, 129, 7, 0), (2, 129, 7, 1), (3, 17, 4, 0)])
def test_fused_chebyshev_cycle_under_sanitizers(orc, tmp_path, dim, npts, levels, mesh):
    """the same sources as one executable with -fsanitize=address,undefined: no report, and the results of the clean build"""
    out, objs = _compile("san", SAN, _sources() + [os.path.join(HERE, "san_cheby.c")])
    exe = os.path.join(out, "san_cheby")
    p = subprocess.run(["g++"] + SAN + ["-o", exe] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    txt = str(tmp_path / "out.txt")
    p = subprocess.run([exe, str(dim), str(npts), str(levels), str(mesh), "-1", str(NCYC), txt], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:]
    got = {ln.split(" ", 1)[0]: ln.split()[1:] for ln in open(txt)}
    ref = _oracle(orc, dim, npts, levels, mesh)
    ref5 = _oracle(orc, dim, npts, levels, mesh, fixed=NCYC)
    assert int(got["solve_iters"][0]) == ref["iters"] and int(got["cycles_iters"][0]) == NCYC
    assert np.abs(np.array(got["solve_rnorm"], dtype=float) / ref["rnorm"] - 1).max() <= 1e-12
    assert np.abs(np.array(got["cycles_rnorm"], dtype=float) / ref5["rnorm"] - 1).max() <= 1e-12
    assert np.array_equal(np.array(got["solve_u"], dtype=float), ref["u"])
    assert np.array_equal(np.array(got["cycles_u"], dtype=float), ref5["u"])
    assert int(got["cycles_calls"][4]) == NCYC                            # the tail stand-in ran once per cycle


def test_chebyshev_needs_fewer_cycles_than_richardson(orc):
    """the motive, on the oracle alone (V(3,3), all levels, rtol 1e-7): Chebyshev (0.2, 2.0) 7 cycles against Richardson + Jacobi (0.8) 9 at
    2-D 129 and 257; 8 against 10 (scale 6/7) at 3-D 33"""
    for dim, npts, levels, scale, want_c, want_r in ((2, 129, 7, 0.8, 7, 9), (2, 257, 8, 0.8, 7, 9), (3, 33, 5, 6.0 / 7.0, 8, 10)):
        r = orc.vcycle(dim, npts, levels, 3, 3, maxiter=100, scale=scale, want_u=False)
        c = orc.vcycle(dim, npts, levels, 3, 3, maxiter=100, ksp_type=1, emin=EIG[0], emax=EIG[1], want_u=False)
        assert c["iters"] < r["iters"], (dim, npts, c["iters"], r["iters"])
        assert (c["iters"], r["iters"]) == (want_c, want_r), (dim, npts, c["iters"], r["iters"])


def test_the_chebyshev_entry_points_are_built_and_kept_out_of_the_mock_linked_host_code():
    """the five kernels are declared and exported by libmgk.so, libmgpetsc.so holds mg_cheby.c; the host sources that the CPU tier links
    against tests/mock_mgk.cpp never name them -- only mg_cheby.c does, and mg_solver.c reaches it through weak references"""
    hk = open(os.path.join(ROOT, "include", "mgk.h")).read()
    assert all(k + "(" in hk for k in KERNELS)
    lib = os.path.join(ROOT, "multigrid_petsc_amd")
    Lk = ctypes.CDLL(os.path.join(lib, "libmgk.so"))
    Lp = ctypes.CDLL(os.path.join(lib, "libmgpetsc.so"))
    assert all(hasattr(Lk, k) for k in KERNELS)
    assert hasattr(Lp, "mg_cheby_pass") and hasattr(Lp, "mg_cheby_tail")
    for f in ("mg_solver.c", "mg_comm.c", "petsc_shim.c", os.path.join("driver", "mgpoisson.c")):
        text = open(os.path.join(CSRC, f)).read()
        for name in KERNELS:
            assert name not in text, f"{f} names {name}"
    text = open(os.path.join(CSRC, "mg_cheby.c")).read()
    assert all(k + "(" in text for k in KERNELS)
    internal = open(os.path.join(CSRC, "mg_solver_internal.h")).read()
    assert internal.count("__attribute__((weak))") >= 2
