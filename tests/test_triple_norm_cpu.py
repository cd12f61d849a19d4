"""CPU tier of the 66-byte 3-D fine level (fuse bit 17, MG_FUSE_TRIPLE_NORM) and of the tuning value that keeps the three-row form of its norm
pass: both stand beside their enums with the next free value, in C and in Python alike; MG_FUSE_AUTO does not contain the bit; mg_solver.c
reaches mg_triple.c's new pass through a weak reference that it tests for NULL, and the kernel ABI has no new entry point; a solver linked
WITHOUT mg_triple.c -- over tests/mock_mgk.cpp, as the other host tests link mg_solver.c -- gives today's results with the bit set.
(Reads files, compiles host code; no GPU.)"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")


def test_the_values_as_a_c_compiler_sees_them(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no host compiler")
    from multigrid_petsc_amd import FUSE_AUTO, FUSE_TRIPLE_MID, FUSE_TRIPLE_NORM, TUNE_J3S_NORM_R3, Fuse, Tune
    src = tmp_path / "v.c"
    src.write_text('#include <stdio.h>\n#include "mgsolve.h"\nint main(void) { printf("%d %d %d %d %d\\n", (int)MG_FUSE_TRIPLE_NORM, (int)MG_FUSE_AUTO, '
                   '(int)MG_FUSE_DEFAULT, (int)MGK_TUNE_J3S_NORM_R3, (int)MGK_TUNE_NO_PROLONG_TRIPLE); return 0; }\n')
    p = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "v")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    bit, auto, default, r3, last = map(int, subprocess.run([str(tmp_path / "v")], check=True, stdout=subprocess.PIPE, text=True).stdout.split())
    assert bit == FUSE_TRIPLE_NORM == 131072 == 2 * FUSE_TRIPLE_MID
    assert auto == FUSE_AUTO and not auto & bit and not default & bit and default == int(Fuse.DEFAULT)          # opt-in
    assert r3 == TUNE_J3S_NORM_R3 == last + 1 == max(int(v) for v in Tune) + 1                                  # the next free value


def test_the_pass_is_a_weak_hook_of_mg_triple_and_the_kernel_abi_is_unchanged():
    internal = open(os.path.join(CSRC, "mg_solver_internal.h")).read()
    assert re.search(r"extern int mg_triple_norm_pass\([^;]*__attribute__\(\(weak\)\);", internal)
    triple = open(os.path.join(CSRC, "mg_triple.c")).read()
    assert re.search(r"^int mg_triple_norm_pass\(", triple, re.M) and "mgk_jacobi3_sumsq_f64(" in triple
    solver = open(os.path.join(CSRC, "mg_solver.c")).read()
    assert "!mg_triple_norm_pass" in solver                                   # tested for NULL before it is called
    mask = internal[internal.index("#define MG_FUSE_POINT_JACOBI_PASSES"):]
    assert "MG_FUSE_TRIPLE_NORM" in mask[:mask.index(")\n")]                  # cleared with the other point-Jacobi passes under a line smoother
    Lp = ctypes.CDLL(os.path.join(ROOT, "multigrid_petsc_amd", "libmgpetsc.so"))
    assert all(hasattr(Lp, n) for n in ("mg_triple_norm_pass", "mg_solver_triple_norm_launches", "mg_solver_graph_rerecorded"))
    from multigrid_petsc_amd.solver import Solver
    assert isinstance(Solver.triple_norm_launches, property) and isinstance(Solver.graph_rerecorded, property)
    # the pass is an entry point the ABI has had: the stand-in of the host tests knows it already
    assert re.search(r"^int mgk_jacobi3_sumsq_f64\(", open(os.path.join(ROOT, "tests", "mock_mgk.cpp")).read(), re.M)


def test_a_build_without_mg_triple_ignores_the_bit(tmp_path):
    """the own driver over tests/mock_mgk.cpp (mg_solver.c + mg_comm.c, no mg_triple.c: the weak references are NULL), 3-D npts 33, 4 levels,
    V(3,3), three cycles: with bits 16 and 17 set and with -1 the stand-in sees the same passes, and the residual history and the field come
    out the same, digit for digit"""
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    from multigrid_petsc_amd import FUSE_AUTO, FUSE_TRIPLE_NORM
    flags = ["-O1", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L", "-I" + os.path.join(ROOT, "include")]
    mock, exe = str(tmp_path / "mock_mgk.o"), str(tmp_path / "mgpoisson")
    for cmd in (["g++", "-std=c++17"] + flags + ["-c", os.path.join(ROOT, "tests", "mock_mgk.cpp"), "-o", mock],
                ["gcc", "-std=c99"] + flags + [os.path.join(CSRC, "driver", "mgpoisson.c"), os.path.join(CSRC, "mg_solver.c"), os.path.join(CSRC, "mg_comm.c"), mock,
                                               "-o", exe, "-lstdc++", "-lm", "-ldl", "-lpthread"]):
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout[-3000:]
    res = {}
    for fuse in (-1, FUSE_AUTO | FUSE_TRIPLE_NORM):
        d = tmp_path / f"fuse{fuse}"
        d.mkdir()
        p = subprocess.run([exe, "-dim", "3", "-npts", "33", "-levels", "4", "-iter", "3", "-ksp_richardson_scale", repr(6.0 / 7.0),
                            "-pc_type", "jacobi", "-mg_fuse", str(fuse), "-write_fields", "1"], cwd=d, env=dict(os.environ, MOCK_MGK_STATS="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0 and "Number of iterations:\t\t3" in p.stdout, p.stdout[-2000:]
        res[fuse] = ((d / "rData.dat").read_text(), (d / "uData.dat").read_text(), re.findall(r"MOCK_MGK_STATS.*", p.stdout))
    assert len(res[-1][1].split()) == 31 ** 3 and res[-1][2]
    assert res[-1] == res[FUSE_AUTO | FUSE_TRIPLE_NORM]
