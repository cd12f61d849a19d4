"""The exact-FMA rule of the fp64 stencil kernels on the CPU (no GPU): tests/exact_fma_check.c checks the host predicate of
csrc/mgk_pow2.h (+-2^e with e >= 0 and nothing else) and that the canonical 7-term sum gives the same bits with the six off-diagonal
terms fused as with multiply + add, on >= 10^6 random tuples for c in {1, 4, 2^20, -2^10}, magnitudes 1e-320 .. 1e300 with signed zeros.
Built with -ffp-contract=off like the product; once more as a stand-alone ASan / UBSan binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "exact_fma_check.c")
INC = "-I" + os.path.join(ROOT, "multigrid_petsc_amd", "csrc")


def _build_and_run(tmp_path, name, flags, args=()):
    exe = str(tmp_path / name)
    p = subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", INC] + flags + [SRC, "-o", exe, "-lm"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return r.stdout


def test_predicate_and_fused_sum_bit_identical(tmp_path):
    out = _build_and_run(tmp_path, "exact_fma_check", [])
    assert out.startswith("ok: 1200000 tuples"), out
    assert " 0 failures" in out


def test_same_program_under_asan_ubsan(tmp_path):
    out = _build_and_run(tmp_path, "exact_fma_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["50000"])
    assert out.startswith("ok: 200000 tuples"), out
    assert "runtime error" not in out and "AddressSanitizer" not in out


@pytest.mark.parametrize("name,value", [("NO_EXACT_FMA", 65)])
def test_forcing_variant_is_named(name, value):
    """the tuning variant that forces the generic form is in the header's enum and in its Python mirror"""
    import re
    from multigrid_petsc_amd import Tune
    txt = open(os.path.join(ROOT, "include", "mgk.h")).read()
    assert re.search(r"\bMGK_TUNE_%s\s*=\s*%d\b" % (name, value), txt)
    assert int(Tune[name]) == value
