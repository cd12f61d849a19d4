"""CPU tier of the prolongation + three-sweep pass (fuse bit 16 in the generic branch of prolong_smooth): its two entry points are declared in
include/mgk_sweep3.h (not in include/mgk.h), exported by libmgk.so and bound in multigrid_petsc_amd/mgk.py; of the host sources only mg_triple.c
names them; mg_solver.c reaches mg_triple.c's two hooks through weak references; the tuning enumerator that switches the pass off takes the
next free value; the fuse masks keep their values.  (Reads files, loads the libraries; no GPU.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
ENTRIES = ("mgk_prolong_jacobi3_f64", "mgk_prolong_jacobi3_ok_f64")
HOOKS = ("mg_triple_prolong_fits", "mg_triple_prolong_pass")


def test_the_entry_points_are_declared_beside_the_abi_header_exported_and_bound():
    h3 = open(os.path.join(ROOT, "include", "mgk_sweep3.h")).read()
    hk = open(os.path.join(ROOT, "include", "mgk.h")).read()
    for name in ENTRIES:
        assert re.search(r"^int\s+%s\(" % name, h3, re.M), name
        assert name not in hk, f"{name} belongs to include/mgk_sweep3.h (the header gates of the tests read include/mgk.h)"
    Lk = ctypes.CDLL(os.path.join(ROOT, "multigrid_petsc_amd", "libmgk.so"))
    assert all(hasattr(Lk, name) for name in ENTRIES)
    Lp = ctypes.CDLL(os.path.join(ROOT, "multigrid_petsc_amd", "libmgpetsc.so"))
    assert all(hasattr(Lp, hook) for hook in HOOKS) and hasattr(Lp, "mg_solver_prolong_triple_launches")
    from multigrid_petsc_amd.mgk import _sigs
    from guarded import _Anything
    table = _sigs(_Anything())
    assert all(name in table for name in ENTRIES)
    assert len(table["mgk_prolong_jacobi3_f64"][1]) == 11 and len(table["mgk_prolong_jacobi3_ok_f64"][1]) == 2
    from multigrid_petsc_amd.solver import Solver
    assert callable(Solver.prolong_triple_launches)


def test_only_mg_triple_names_the_entry_points_and_the_hooks_are_weak():
    for f in sorted(os.listdir(CSRC)) + [os.path.join("driver", "mgpoisson.c")]:
        if not f.endswith(".c") or f == "mg_triple.c":
            continue
        text = open(os.path.join(CSRC, f)).read()
        for name in ENTRIES:
            assert name not in text, f"{f} names {name}"
    text = open(os.path.join(CSRC, "mg_triple.c")).read()
    assert all(name + "(" in text for name in ENTRIES)
    internal = open(os.path.join(CSRC, "mg_solver_internal.h")).read()
    for hook in HOOKS:
        assert re.search(r"extern int %s\([^;]*__attribute__\(\(weak\)\);" % hook, internal), hook
        assert re.search(r"^int %s\(" % hook, text, re.M), hook
    solver = open(os.path.join(CSRC, "mg_solver.c")).read()
    assert "!mg_triple_prolong_pass || !mg_triple_prolong_fits" in solver          # tested for NULL before they are called


def test_the_switch_takes_the_next_free_value_and_the_masks_stay():
    from multigrid_petsc_amd import FUSE_AUTO, FUSE_TRIPLE_MID, Fuse, Tune
    hk = open(os.path.join(ROOT, "include", "mgk.h")).read()
    body = re.search(r"enum mgk_tune \{(.*?)\}", hk, flags=re.S).group(1)
    values = {n: int(v) for n, v in re.findall(r"\bMGK_TUNE_([A-Z0-9_]+)\s*=\s*(-?\d+)", body)}
    assert values["NO_PROLONG_TRIPLE"] == int(Tune.NO_PROLONG_TRIPLE) == max(values.values()) == 69
    assert sorted(values.values()).count(69) == 1
    assert FUSE_TRIPLE_MID == 65536 and FUSE_AUTO == int(Fuse.DEFAULT) | FUSE_TRIPLE_MID
    hs = open(os.path.join(ROOT, "include", "mgsolve.h")).read()
    assert "#define MG_FUSE_TRIPLE_MID 65536" in hs and "#define MG_FUSE_AUTO (MG_FUSE_DEFAULT | MG_FUSE_TRIPLE_MID)" in hs
