"""mg_config.line_tail (the LDS-resident coarse levels of a line cycle in one launch), CPU tier.  The product's mg_solver.c + mg_comm.c +
mg_line.c + mg_xline.c + mg_line_tail.c over host-memory stand-ins (tests/mock_mgk_line_tail.cpp, which includes tests/mock_mgk_xline.cpp
textually and builds mgk_tail_cycle_line_f64 from the stand-ins' own per-pass functions), driven through Solver(..., line_tail=1):

  solves        every case of tests/xline_reference.py and the y cases of tests/line_reference.py: the pinned count, the history within 1e-12
                of rnorm[0], u bit for bit; count, history and u EQUAL to the same solve with line_tail=0; graph=0 and fuse=0 give the same
                bits; reset + solve repeats them (in the worker); dof_updates_per_cycle unchanged
  launches      the log of executed passes: per cycle the line passes of the levels above tail_level going down, ONE tail call, the same
                passes going up -- no line pass on a level >= tail_level; with line_tail=0 no tail call at all
  tail_level    the first level with n <= 63 (1 up to npts 129, 2 at 257); 0 with line_tail=0, with fewer than two levels left, with v0 = 0
  refusals      line_tail = 2, -1; line_tail = 1 with point Jacobi; in a link without mg_line_tail.c line_tail = 1 is refused with a message
                and line_tail = 0 runs to the same bits
  sanitizers    the same sources as a plain executable (tests/san_line_tail.c) under -fsanitize=address,undefined, refusals and leaks included"""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import line_reference as LR
import xline_reference as XR
from oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
KERNEL = "mgk_tail_cycle_line_f64"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
YCASES = [("yline",) + c + (None,) for c in LR.CASES]
CASES = list(XR.CASES) + YCASES
IDS = [XR.xcase_key(c) for c in CASES]
SAN_CASES = [XR.CASES[4], XR.CASES[10], XR.CASES[17], YCASES[9]]      # altline mesh 2, altline mesh 1 (rough), xline mesh 1 (rough), yline mesh 2 (rough)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _reference(orc, case):
    return LR.reference(orc, case[1:5]) if case[0] == "yline" else XR.reference(orc, case)


def _compile(tag, extra, sources):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src in sources:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"linetail_{tag}_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + extra + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    return out, objs


def _sources(mock="mock_mgk_line_tail.cpp", tail=True):
    return [os.path.join(HERE, mock)] + [os.path.join(CSRC, f) for f in ("mg_solver.c", "mg_comm.c", "mg_line.c", "mg_xline.c")] + \
           ([os.path.join(CSRC, "mg_line_tail.c")] if tail else [])


def _link(out, objs, name):
    so = os.path.join(out, name)
    p = subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return so


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through Solver in one worker process (the loader caches its libraries)"""
    out, objs = _compile("plain", [], _sources())
    so = _link(out, objs, "libmgsolve_linetail_mock.so")
    npz = str(tmp_path_factory.mktemp("linetail") / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "line_tail_mock_worker.py"), so, npz] + IDS,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(npz)


def _sweeps(pc, count):
    """the stand-ins' letters of one smoothing: a y sweep is f b, an x sweep F B"""
    return "".join("FB" if pc == "xline" or (pc == "altline" and k % 2) else "fb" for k in range(count))


def _tail_level(npts, levels):
    return next(l for l in range(1, levels) if (npts - 1) // 2 ** l - 1 <= 63)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_solve_with_the_tail_equals_the_reference_and_the_launches(orc, results, case):
    k = XR.xcase_key(case) + ":"
    pc, npts, levels = case[0], case[1], case[2]
    ref = _reference(orc, case)
    if case[5] is not None:
        assert ref["iters"] == case[5]
    it = int(results[k + "it"])
    XR.compare(ref, it, results[k + "rn"], results[k + "u"], float(results[k + "bnorm"]))
    t = _tail_level(npts, levels)
    assert int(results[k + "tail_level"]) == t == (2 if npts == 257 else 1) and int(results[k + "off_tail_level"]) == 0
    for tag in ("off", "graph0", "fuse0"):
        assert int(results[k + tag + "_it"]) == it, tag
        assert np.array_equal(results[k + tag + "_rn"], results[k + "rn"]) and np.array_equal(results[k + tag + "_u"], results[k + "u"]), tag
        assert float(results[k + tag + "_dof"]) == float(results[k + "dof"])
        assert int(results[k + tag + "_tail_level"]) == (0 if tag == "off" else t)
    # one tail call per cycle; line passes on the levels above tail_level alone
    cycle = _sweeps(pc, 3) * t + "T" + _sweeps(pc, 3) * t
    assert str(results[k + "log"]) == cycle * it
    assert str(results[k + "graph0_log"]) == cycle * it and str(results[k + "fuse0_log"]) == cycle * it
    full = _sweeps(pc, 3) * (2 * (levels - 1) + 1)
    assert str(results[k + "off_log"]) == full * it


@pytest.mark.parametrize("v", [(2, 1), (1, 2)])
def test_other_sweep_counts(orc, results, v):
    """(altline, 33, 5, 2): v0 sweeps above the coarsest level, v1 on it, each smoothing counted from 0 -- inside the tail too"""
    h = XR.Hierarchy(orc, 33, 5, 2, "altline")
    ref = XR.solve(h, h.rhs(), XR.SCALE, v=v, rtol=XR.RTOL, maxiter=100)
    on, off = f"v:{v[0]},{v[1]},1:", f"v:{v[0]},{v[1]},0:"
    assert int(results[on + "it"]) == int(results[off + "it"]) == ref["iters"]
    assert np.array_equal(results[on + "u"], ref["u"]) and np.array_equal(results[off + "u"], ref["u"])
    assert np.array_equal(results[on + "rn"], results[off + "rn"])
    assert np.abs(results[on + "rn"] - ref["rnorm"]).max() <= 1e-12 * ref["rnorm"][0]
    assert int(results[on + "tail_level"]) == 1 and int(results[off + "tail_level"]) == 0
    assert str(results[on + "log"]) == (_sweeps("altline", v[0]) + "T" + _sweeps("altline", v[0])) * ref["iters"]
    assert str(results[off + "log"]) == (_sweeps("altline", v[0]) * 4 + _sweeps("altline", v[1]) + _sweeps("altline", v[0]) * 4) * ref["iters"]


def test_fall_backs_and_the_accessor(results):
    """line_tail = 1 is accepted and the tail stays off where fewer than two levels would be left or nothing is pre-smoothed; the accessor
    shows point Jacobi's tail (fuse bit 9) as well; every tail call was counted"""
    for tag in ("two", "v0"):
        on, off = f"fallback:{tag},1:", f"fallback:{tag},0:"
        assert int(results[on + "tail_level"]) == 0 and int(results[off + "tail_level"]) == 0
        assert int(results[on + "it"]) == int(results[off + "it"]) >= 1
        assert np.array_equal(results[on + "rn"], results[off + "rn"]) and np.array_equal(results[on + "u"], results[off + "u"])
    assert int(results["jacobi_tail_level"]) == 1
    assert int(results["tail_calls"]) > 0


def test_a_library_without_mg_line_tail_links_and_refuses(orc, results, tmp_path):
    """the x-line tier's link (mock_mgk_xline.cpp + mg_solver.c + mg_comm.c + mg_line.c + mg_xline.c): no strong reference to anything new"""
    out, objs = _compile("notail", [], _sources("mock_mgk_xline.cpp", tail=False))
    so = _link(out, objs, "libmgsolve_nolinetail_mock.so")
    lib = ctypes.CDLL(so)
    assert not hasattr(lib, "mg_line_tail") and not hasattr(lib, KERNEL) and hasattr(lib, "mg_xline_smooth")
    npz = str(tmp_path / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "line_tail_mock_worker.py"), so, npz, "--without-mg-line-tail"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    r = np.load(npz)
    k = "altline,33,5,2,manufactured:"
    assert int(r["tail_level"]) == 0
    assert int(r["it"]) == int(results[k + "it"]) and np.array_equal(r["rn"], results[k + "rn"]) and np.array_equal(r["u"], results[k + "u"])


@pytest.fixture(scope="module")
def san_exe():
    """the same sources as one executable with -fsanitize=address,undefined, built once"""
    out, objs = _compile("san", SAN, _sources() + [os.path.join(HERE, "san_line_tail.c")])
    exe = os.path.join(out, "san_line_tail")
    p = subprocess.run(["g++"] + SAN + ["-o", exe] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("case", SAN_CASES, ids=[XR.xcase_key(c) for c in SAN_CASES])
def test_solve_under_sanitizers(orc, san_exe, tmp_path, case):
    """under -fsanitize=address,undefined: no report (leaks included), the refusals, and results that pass the same bars with and without the tail"""
    pc, npts, levels, mesh, rhs = case[:5]
    ref = _reference(orc, case)
    rhsfile = "-"
    if rhs != "manufactured":
        import rhs_cases
        rhsfile = str(tmp_path / "rhs.bin")
        rhs_cases.uniform(2, npts, int(rhs.split(":")[1])).tofile(rhsfile)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    txt = str(tmp_path / "out.txt")
    p = subprocess.run([san_exe, {"yline": "1", "xline": "2", "altline": "3"}[pc], str(npts), str(levels), str(mesh), repr(XR.SCALE), rhsfile, txt],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:]
    got = {ln.split(" ", 1)[0]: ln.split()[1:] for ln in open(txt)}
    for tag in ("solve", "again", "plain"):
        rn = np.array(got[tag + "_rnorm"], dtype=float)
        XR.compare(ref, int(got[tag + "_iters"][0]), rn, np.array(got[tag + "_u"], dtype=float), ref["bnorm"])
        assert int(got[tag + "_tail_level"][0]) == (0 if tag == "plain" else 1)
    assert got["solve_rnorm"] == got["plain_rnorm"] and got["solve_u"] == got["plain_u"]


def test_the_entry_point_is_built_and_only_mg_line_tail_names_the_kernel():
    """the kernel is declared and exported by libmgk.so, the hook and the accessor by libmgpetsc.so; of the host sources only mg_line_tail.c
    names the kernel; mg_config and MgConfig carry the field directly before the two chunk periods (which stay last), off by default; the
    driver takes -line_tail"""
    hk, hs = open(os.path.join(ROOT, "include", "mgk.h")).read(), open(os.path.join(ROOT, "include", "mgsolve.h")).read()
    assert KERNEL + "(" in hk and hs.index("int pc_type;") < hs.index("int line_tail;") < hs.index("int xline_chunk;") < hs.index("int line_chunk;")
    assert "int  mg_solver_tail_level(const mg_solver *s);" in hs
    lib = os.path.join(ROOT, "multigrid_petsc_amd")
    Lk = ctypes.CDLL(os.path.join(lib, "libmgk.so"))
    Lp = ctypes.CDLL(os.path.join(lib, "libmgpetsc.so"))
    assert hasattr(Lk, KERNEL) and hasattr(Lp, "mg_line_tail") and hasattr(Lp, "mg_solver_tail_level")
    for f in sorted(os.listdir(CSRC)) + [os.path.join("driver", "mgpoisson.c")]:
        if f.endswith(".c") and f != "mg_line_tail.c":
            assert KERNEL not in open(os.path.join(CSRC, f)).read(), f"{f} names {KERNEL}"
    assert KERNEL + "(" in open(os.path.join(CSRC, "mg_line_tail.c")).read()
    from multigrid_petsc_amd.solver import MgConfig
    assert [f[0] for f in MgConfig._fields_][-4:] == ["pc_type", "line_tail", "xline_chunk", "line_chunk"]      # as the header has them
    cfg = MgConfig()
    cfg.line_tail = 7
    Lp.mg_config_default(ctypes.byref(cfg))
    assert cfg.line_tail == 0 and cfg.line_chunk == 0
    assert '"-line_tail"))) c.line_tail = atoi(v)' in open(os.path.join(CSRC, "driver", "mgpoisson.c")).read()
    from multigrid_petsc_amd.mgk import _sigs  # noqa: F401  (the binding lists the entry point)
    assert '"mgk_tail_cycle_line_f64"' in open(os.path.join(lib, "mgk.py")).read()
