"""CPU tier of the 75-byte 3-D fine level (fuse bit 16, MG_FUSE_TRIPLE_MID): the two entry points of the stacked three-sweep pass are declared
in include/mgk_sweep3.h (not in include/mgk.h) and exported by libmgk.so; of the host sources only mg_triple.c names them; and a solver linked
WITHOUT mg_triple.c -- over tests/mock_mgk.cpp, as the other host tests link mg_solver.c -- runs today's passes and gives today's results with
the bit set.  (Reads files, compiles host code; no GPU.)"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
ENTRIES = ("mgk_jacobi3_sumsq_mid_f64", "mgk_jacobi3_mid_ok_f64")


def test_the_entry_points_are_declared_beside_the_abi_header_and_exported():
    h3 = open(os.path.join(ROOT, "include", "mgk_sweep3.h")).read()
    hk = open(os.path.join(ROOT, "include", "mgk.h")).read()
    for name in ENTRIES:
        assert re.search(r"^int\s+%s\(" % name, h3, re.M), name
        assert name not in hk, f"{name} belongs to include/mgk_sweep3.h (the header gates of the tests read include/mgk.h)"
    # the conventions are stated where the functions are declared
    flat = re.sub(r"\s*\n\s*\*\s*", " ", h3)
    for phrase in ("nothing outside the interior of unew is written", "read as zeros", "unew must not be u or b"):
        assert phrase in flat, phrase
    Lk = ctypes.CDLL(os.path.join(ROOT, "multigrid_petsc_amd", "libmgk.so"))
    assert all(hasattr(Lk, name) for name in ENTRIES)
    Lp = ctypes.CDLL(os.path.join(ROOT, "multigrid_petsc_amd", "libmgpetsc.so"))
    assert hasattr(Lp, "mg_triple_mid_pass") and hasattr(Lp, "mg_triple_mid_fits")
    from multigrid_petsc_amd.mgk import _sigs
    from guarded import _Anything
    assert all(name in _sigs(_Anything()) for name in ENTRIES)          # bound in multigrid_petsc_amd/mgk.py


def test_only_mg_triple_names_the_entry_points():
    for f in sorted(os.listdir(CSRC)) + [os.path.join("driver", "mgpoisson.c")]:
        if not f.endswith(".c") or f == "mg_triple.c":
            continue
        text = open(os.path.join(CSRC, f)).read()
        for name in ENTRIES:
            assert name not in text, f"{f} names {name}"
    text = open(os.path.join(CSRC, "mg_triple.c")).read()
    assert all(name + "(" in text for name in ENTRIES)
    internal = open(os.path.join(CSRC, "mg_solver_internal.h")).read()
    for hook in ("mg_triple_mid_fits", "mg_triple_mid_pass"):
        assert re.search(r"extern int %s\([^;]*__attribute__\(\(weak\)\);" % hook, internal), hook


def test_the_bit_stands_beside_the_enum_and_minus_one_selects_it():
    """MG_FUSE_TRIPLE_MID = 65536 and MG_FUSE_AUTO = MG_FUSE_DEFAULT | MG_FUSE_TRIPLE_MID, as a C compiler evaluates them, equal the Python
    constants; MG_FUSE_DEFAULT keeps its value"""
    if shutil.which("gcc") is None:
        pytest.skip("no host compiler")
    import tempfile
    from multigrid_petsc_amd import FUSE_AUTO, FUSE_TRIPLE_MID, Fuse
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "bit.c")
        open(src, "w").write('#include <stdio.h>\n#include "mgsolve.h"\nint main(void) { printf("%d %d %d\\n", (int)MG_FUSE_TRIPLE_MID, (int)MG_FUSE_AUTO, (int)MG_FUSE_DEFAULT); return 0; }\n')
        p = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "bit")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout
        bit, auto, default = map(int, subprocess.run([os.path.join(d, "bit")], check=True, stdout=subprocess.PIPE, text=True).stdout.split())
    assert bit == FUSE_TRIPLE_MID == 65536 and auto == FUSE_AUTO == default | bit and default == int(Fuse.DEFAULT) and not default & bit
    assert "s->cfg.fuse = MG_FUSE_AUTO" in open(os.path.join(CSRC, "mg_solver.c")).read()


def test_a_build_without_mg_triple_runs_todays_passes(tmp_path):
    """the own driver over tests/mock_mgk.cpp (mg_solver.c + mg_comm.c, no mg_triple.c: the weak references are NULL), 3-D npts 33, 4 levels,
    V(3,3), three cycles: with the bit set, with the default mask without it and with -1 the stand-in sees the same passes, and the residual
    history and the field come out the same, digit for digit"""
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    from multigrid_petsc_amd import FUSE_TRIPLE_MID, Fuse
    out = os.path.join(ROOT, "tests", "_san")
    os.makedirs(out, exist_ok=True)
    flags = ["-O1", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L", "-I" + os.path.join(ROOT, "include")]
    mock = os.path.join(out, "triple_mock_mgk.o")
    for cmd in (["g++", "-std=c++17"] + flags + ["-c", os.path.join(ROOT, "tests", "mock_mgk.cpp"), "-o", mock],
                ["gcc", "-std=c99"] + flags + [os.path.join(CSRC, "driver", "mgpoisson.c"), os.path.join(CSRC, "mg_solver.c"), os.path.join(CSRC, "mg_comm.c"), mock,
                                               "-o", os.path.join(out, "triple_mgpoisson"), "-lstdc++", "-lm", "-ldl", "-lpthread"]):
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout[-3000:]
    res = {}
    for fuse in (-1, int(Fuse.DEFAULT), int(Fuse.DEFAULT) | FUSE_TRIPLE_MID):
        d = tmp_path / f"fuse{fuse}"
        d.mkdir()
        p = subprocess.run([os.path.join(out, "triple_mgpoisson"), "-dim", "3", "-npts", "33", "-levels", "4", "-iter", "3", "-ksp_richardson_scale", repr(6.0 / 7.0),
                            "-pc_type", "jacobi", "-mg_fuse", str(fuse), "-write_fields", "1"], cwd=d, env=dict(os.environ, MOCK_MGK_STATS="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0 and "Number of iterations:\t\t3" in p.stdout, p.stdout[-2000:]
        res[fuse] = ((d / "rData.dat").read_text(), (d / "uData.dat").read_text(), re.findall(r"MOCK_MGK_STATS.*", p.stdout))
    assert len(res[-1][0].split()) == 4 and len(res[-1][1].split()) == 31 ** 3 and res[-1][2]
    assert res[int(Fuse.DEFAULT)] == res[-1] == res[int(Fuse.DEFAULT) | FUSE_TRIPLE_MID]
