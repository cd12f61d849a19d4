"""CPU tier of tests/test_random_sessions_gpu.py: whole solver sessions drawn at random (fixed seeds) on the product's HOST logic over the
host-memory stand-ins of the kernel ABI -- one Solver and a sequence of operations on the same live handle, every result compared with a
reference that starts afresh (tools/stress_sessions_mock.py, which says what is drawn and how it is judged).

  (a) the draw: 300 point-Jacobi sessions (solve, cycles, fmg, solve_fmg, solve_gmres, right-hand-side changes; mg_solver.c + mg_comm.c +
      mg_fmg.c + mg_gmres.c over tests/mock_mgk_fmg.cpp) and 300 line-smoother sessions (yline / xline / altline with line_chunk / xline_chunk;
      mg_solver.c + mg_comm.c + mg_line.c + mg_xline.c + mg_line_chunk.c + mg_xline_chunk.c over tests/mock_mgk_xchunkline.cpp), each in a
      process of its own over its own library under tests/_san/: 0 mismatches, 0 refused
  (b) the four FMG stand-ins against the restatement (tests/fmg_reference.py), kernel by kernel and bit for bit: a wrong mock would make the
      draw agree with the wrong thing
  (c) tests/san_fmg.c: fixed FMG sessions as a plain executable under -fsanitize=address,undefined (mg_solver.c + mg_comm.c + mg_fmg.c +
      tests/mock_mgk_fmg.cpp), with the tail kernel and without it, 2-D 65 / 6 levels and 3-D 17 / 3 levels: no report, no leak, the refusals,
      and every field and history equal to the restatement's (fields bit for bit)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from fmg_reference import FmgRef
from oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "stress_sessions_mock.py")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
NO_TAIL = 63 | 256 | 1024 | 2048 | 4096 | 8192 | 16384      # the default fuse bits without bit 9 (the tail kernel)
# (dim, npts, levels, v, scale, fuse, pair_min_n)
SAN_CASES = [(2, 65, 6, (3, 3), 0.8, -1, 0), (2, 65, 6, (3, 3), 0.8, NO_TAIL, 0), (2, 65, 6, (1, 2), 0.8, NO_TAIL, 0), (2, 65, 6, (4, 1), 1.0, -1, 0),
             (3, 17, 3, (3, 3), 6.0 / 7.0, -1, 0), (3, 17, 3, (3, 3), 6.0 / 7.0, NO_TAIL, 0), (3, 17, 3, (2, 3), 0.8, NO_TAIL, 0),
             # found by the draw with mg_fmg.c's swap back to the recorded buffer roles taken out (sessions 756 and 562 of `1000 5 point`): no
             # tail, the graph on, a stage level that swaps u / tmp an odd number of times, and a replay of the recording after a second FMG
             (2, 33, 5, (4, 1), 6.0 / 7.0, 507, 31), (3, 33, 5, (4, 2), 0.8, 32063, 15)]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _tool():
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import stress_sessions_mock
    return stress_sessions_mock


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind,seed", [("point", 7), ("line", 7)])
def test_random_sessions_on_the_host_mock_equal_their_references(kind, seed):
    """(a).  The library lands in tests/_san/ (git-ignored); the draw runs in a worker process, because the loader caches what it hands out"""
    so = _tool().build_mock(kind)
    assert os.path.dirname(so) == os.path.join(HERE, "_san")
    p = subprocess.run([sys.executable, TOOL, "300", str(seed), kind], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=800, cwd=ROOT)
    assert p.returncode == 0 and "300 sessions, 0 mismatches, 0 refused" in p.stdout, p.stdout[-4000:]
    assert "MISMATCH" not in p.stdout and "REFUSED" not in p.stdout, p.stdout[-4000:]


@pytest.fixture(scope="module")
def standins(tmp_path_factory):
    so = _tool().build_mock("point")
    npz = str(tmp_path_factory.mktemp("fmgmock") / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "fmg_mock_worker.py"), so, npz], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(npz)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("v", [(3, 3), (1, 2), (5, 1)])
def test_tail_fmg_stand_in_equals_the_restatement(orc, standins, dim, nu, v):
    """(b): mgk_tail_fmg_f64 of the mock on the stacks 63 .. 1 (2-D) and 15 .. 1 (3-D)"""
    n0, nlev = (63, 6) if dim == 2 else (15, 4)
    key = f"tail:{dim}:{nu}:{v[0]}:{v[1]}"
    f = FmgRef(orc, dim, n0 + 2, nlev, v, 0.8 if dim == 2 else 6.0 / 7.0, b0=standins[key + ":b"])
    assert np.array_equal(standins[key + ":u"], f.fmg(nu)), key
    assert int(standins["ghosts:" + key]) == 1


@pytest.mark.parametrize("dim,n,sweeps", [(2, 31, 3), (3, 15, 2)])
def test_interpolation_stand_ins_equal_the_restatement(orc, standins, dim, n, sweeps):
    """(b): mgk_interp_jacobi3_2d_f64 / mgk_interp_jacobi2_f64 of the mock: a zeroed field + P uc, then three / two sweeps; the output's old
    contents (NaN) are never read"""
    key = f"interp:{dim}"
    b, uc = standins[key + ":b"], standins[key + ":uc"]
    As = orc.level_stencil(dim, n + 2, 0)[0]
    sc = 0.8 if dim == 2 else 6.0 / 7.0
    u = orc.prolong_add(dim, n, uc, np.zeros(n ** dim))
    for _ in range(sweeps):
        u = orc.jacobi(dim, n, As, sc, b, u)
    assert np.array_equal(standins[key + ":u"], u), key
    assert int(standins["ghosts:" + key]) == 1


@pytest.fixture(scope="module")
def san_exe():
    """mg_solver.c + mg_comm.c + mg_fmg.c + the stand-ins + tests/san_fmg.c as one executable with -fsanitize=address,undefined, built once"""
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src in [os.path.join(HERE, "mock_mgk_fmg.cpp"), os.path.join(CSRC, "mg_solver.c"), os.path.join(CSRC, "mg_comm.c"), os.path.join(CSRC, "mg_fmg.c"),
                os.path.join(HERE, "san_fmg.c")]:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"sessions_san_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + SAN + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    exe = os.path.join(out, "san_fmg")
    p = subprocess.run(["g++"] + SAN + ["-o", exe] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.timeout(900)
@pytest.mark.parametrize("dim,npts,levels,v,scale,fuse,pair", SAN_CASES)
def test_fmg_sessions_under_sanitizers(orc, san_exe, tmp_path, dim, npts, levels, v, scale, fuse, pair):
    """(c): the program is run directly; a sanitizer or leak report is a non-zero exit status (exitcode=99), a missed refusal or a handle that
    differs after the refusals is one too"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    txt = str(tmp_path / "out.txt")
    p = subprocess.run([san_exe, str(dim), str(npts), str(levels), str(v[0]), str(v[1]), repr(scale), str(fuse), str(pair), txt], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=800)
    assert p.returncode == 0, p.stdout[-4000:]
    got = {ln.split(" ", 1)[0]: np.array(ln.split()[1:], dtype=float) for ln in open(txt)}
    f = FmgRef(orc, dim, npts, levels, v, scale)
    plain = orc.vcycle(dim, npts, levels, v[0], v[1], maxiter=40, scale=scale)
    it, u, rn = f.solve_fmg(1, maxiter=40, rtol=1e-7)
    want = {"fmg1c3": f.fmg_then_cycles(1, 3), "fmg2": f.fmg_then_cycles(2, 0), "fmg2c3": f.fmg_then_cycles(2, 3), "fmg2c1": f.fmg_then_cycles(2, 1),
            "fmg1": f.fmg_then_cycles(1, 0), "fmg1c2": f.fmg_then_cycles(1, 2), "solve_fmg2c3": f.fmg_then_cycles(2, 3),
            "again": f.fmg_then_cycles(1, 0), "sfmg1": (u, rn), "solve": (plain["u"], plain["rnorm"]), "after": (plain["u"], plain["rnorm"])}
    for tag, (u, rn) in want.items():
        assert int(got[tag + "_iters"][0]) == len(rn) - 1 == len(got[tag + "_rnorm"]) - 1, tag
        assert np.array_equal(got[tag + "_u"], u), tag
        assert np.max(np.abs(got[tag + "_rnorm"] - rn) / rn) <= 1e-10, tag
        assert abs(got[tag + "_bnorm"][0] - f.bnorm()) <= 1e-12 * f.bnorm(), tag
    assert it == int(got["sfmg1_iters"][0])
