"""CPU tier of the stacked 3-D pass's load policy: the tuning value that restores the non-temporal loads of b,
MGK_TUNE_J3S_B_NT, stands beside the enum with the next free number, in C and in Python alike, and the enum and Tune are what they were; the
launcher reads it in one place and the kernel ABI has no new entry point.  (The tile order of the pass did not change -- the ty-fastest order
lost its gate, profiles/stacked_l2/README.md -- so there is no decode to check on the host.)  (Reads files, compiles host code; no GPU.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")


def test_the_value_as_a_c_compiler_sees_it(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no host compiler")
    import multigrid_petsc_amd
    from multigrid_petsc_amd import TUNE_J3S_B_NT, TUNE_J3S_NORM_R3, Tune
    src = tmp_path / "v.c"
    src.write_text('#include <stdio.h>\n#include "mgk.h"\nint main(void) { printf("%d %d %d\\n", (int)MGK_TUNE_J3S_B_NT, (int)MGK_TUNE_J3S_NORM_R3, '
                   '(int)MGK_TUNE_NO_PROLONG_TRIPLE); return 0; }\n')
    p = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "v")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    bnt, r3, last = map(int, subprocess.run([str(tmp_path / "v")], check=True, stdout=subprocess.PIPE, text=True).stdout.split())
    assert last == max(int(v) for v in Tune) == 69                  # the enum and Tune end where they did
    assert r3 == TUNE_J3S_NORM_R3 == last + 1
    assert bnt == TUNE_J3S_B_NT == last + 2 == 71                   # the next free value
    assert multigrid_petsc_amd.mgk.TUNE_J3S_B_NT == 71
    # beside the enum, not inside it: every value past the last enumerator is a #define
    header = open(os.path.join(ROOT, "include", "mgk.h")).read()
    defines = dict(re.findall(r"^#define (MGK_TUNE_\w+) (\d+)$", header, re.M))
    assert defines == {"MGK_TUNE_J3S_NORM_R3": "70", "MGK_TUNE_J3S_B_NT": "71"}
    enum = header[header.index("enum mgk_tune"):]
    assert "J3S_B_NT" not in enum[:enum.index("};")]


def test_one_reader_and_no_new_entry_point():
    unit = open(os.path.join(CSRC, "mgk_sweep3.hip")).read()
    assert len(re.findall(r"g_variant == MGK_TUNE_J3S_B_NT", unit)) == 1
    others = [f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".c", ".h")) and f != "mgk_sweep3.hip"]
    assert not any("MGK_TUNE_J3S_B_NT" in open(os.path.join(CSRC, f)).read() for f in others)
    # the policy is a template argument of the one kernel: no second entry point, no new function of include/mgk.h
    assert len(re.findall(r"^__global__ void __launch_bounds__\(64 \* J3S_WAVES\) k_jacobi3s\(", unit, re.M)) == 1
    assert not re.search(r"__global__[^\n]*k_jacobi3s\w+\(", unit)
