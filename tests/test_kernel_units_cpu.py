"""The layout of libmgk.so's translation units (csrc/*.hip), read from the sources: no GPU and no compiler needed.

Every unit is built (it is an object of the Makefile's KOBJ, and KOBJ names nothing else) and every unit's code object is loaded when a
context is created: exactly one MGK_PRELOAD_UNIT(...) line per unit (csrc/mgk_dev.hpp), and no preload function of the old kind."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")


def _units():
    units = sorted(os.path.basename(p)[:-len(".hip")] for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(units) >= 2, units
    return units


def _kobj():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.findall(r"^KOBJ\s*=(.*)$", text, flags=re.M)
    assert len(m) == 1, m
    objs = m[0].split()
    assert all(o.endswith(".o") for o in objs), objs
    return [o[:-len(".o")] for o in objs]


def test_every_unit_is_an_object_of_the_library_and_every_object_a_unit():
    kobj = _kobj()
    assert len(kobj) == len(set(kobj)), kobj
    assert sorted(kobj) == _units()


def test_every_unit_registers_exactly_one_preload_kernel():
    for u in _units():
        lines = [l for l in open(os.path.join(CSRC, u + ".hip")).read().split("\n") if "MGK_PRELOAD_UNIT(" in l]
        assert len(lines) == 1, (u, lines)
        assert re.match(r"MGK_PRELOAD_UNIT\(\S.*\)\s*$", lines[0]), (u, lines[0])      # at file scope, naming a kernel


def test_no_unit_declares_a_preload_function():
    for u in _units():
        assert "mgk_preload_" not in open(os.path.join(CSRC, u + ".hip")).read(), u
