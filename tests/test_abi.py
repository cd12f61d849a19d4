"""CPU tests of the product's C ABI: the libraries load without a GPU, export every symbol the headers
declare, refuse to run without a device (no CPU fallback), and the integer host logic is right."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header, prefix):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[A-Za-z0-9_]+)\s*\(" % prefix, txt)))


def test_libmgk_exports_every_declared_symbol():
    from multigrid_petsc_amd._lib import load_mgk
    L = load_mgk()
    names = _declared("mgk.h", "mgk_")
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), f"libmgk.so does not export {n}"


def test_libmgpetsc_exports_every_declared_symbol():
    from multigrid_petsc_amd._lib import load_mgpetsc
    L = load_mgpetsc()
    names = _declared("mgsolve.h", "mg_") + _declared("mg_comm.h", "mg_comm_")
    assert len(names) >= 25
    for n in set(names):
        assert hasattr(L, n), f"libmgpetsc.so does not export {n}"


def test_geometry_layout():
    from multigrid_petsc_amd.mgk import Geom, _sigs
    from multigrid_petsc_amd._lib import load_mgk
    L = load_mgk()
    _sigs(L)
    g = Geom()
    assert L.mgk_geom_init(C.byref(g), 3, 1023, 1023, 1023) == 0
    assert g.pitch == 1040 and g.pitch % 16 == 0            # 16 + 1024 doubles: whole 128-B lines
    assert g.plane == 1040 * 1025 and g.org == g.plane + g.pitch + 16
    assert g.total == g.plane * 1025 + g.pitch
    assert L.mgk_geom_init(C.byref(g), 2, 4095, 4095, 1) == 0
    assert g.pitch == 4112 and g.nz == 1 and g.org == g.pitch + 16
    assert L.mgk_geom_init(C.byref(g), 3, 4, 4, 4) != 0     # even nx is rejected
    assert L.mgk_geom_init(C.byref(g), 4, 3, 3, 3) != 0


def test_no_cpu_fallback_without_a_device():
    from multigrid_petsc_amd.mgk import Mgk, MgkError
    from multigrid_petsc_amd._lib import load_mgk
    if load_mgk().mgk_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(MgkError, match="no HIP device"):
        Mgk(0)
    from multigrid_petsc_amd.solver import Solver, MgError
    with pytest.raises(MgError):
        Solver(2, 17, 2)


def test_ranges_and_maps_match_reference_semantics():
    from multigrid_petsc_amd import solver as S
    from oracle import Oracle
    orc = Oracle()
    L = S._lib()
    for tot, procs in ((225, 1), (16129, 8), (9, 8), (49, 3), (1070599167, 8)):
        want = np.zeros(procs + 1, dtype=np.int32)
        orc.L.mgo_get_ranges(tot, procs, want.ctypes.data)
        assert np.array_equal(S.get_ranges(tot, procs), want)
    for npts in (17, 129, 1025):
        for g in range(4):
            assert L.mg_grid_n(npts, g) == orc.L.mgo_grid_n(npts, g)
    k, i, j = C.c_int(), C.c_int(), C.c_int()
    for dim, n in ((2, 15), (3, 7)):
        for idx in (0, 1, n, n * n - 1, n ** dim - 1):
            L.mg_global_to_grid(dim, n, idx, C.byref(k), C.byref(i), C.byref(j))
            assert L.mg_grid_to_global(dim, n, k.value, i.value, j.value) == idx


@pytest.mark.parametrize("npts,ldist,nranks", [(1025, 4, 8), (1025, 4, 2), (1025, 3, 4), (513, 3, 8), (129, 1, 3), (65, 2, 5)])
def test_slab_split_is_nested_and_covers(npts, ldist, nranks):
    """multi-GPU decomposition: slabs tile every distributed level, starts are even, and the slab of level l
    is exactly twice the slab of level l+1 (+ the one extra plane on the last rank)."""
    from multigrid_petsc_amd.solver import slab_range, _lib
    L = _lib()
    for l in range(ldist + 1):
        n = L.mg_grid_n(npts, l)
        prev_end = 0
        for r in range(nranks):
            a, b = slab_range(npts, ldist, l, r, nranks)
            assert a == prev_end and b > a
            if l < ldist:
                assert a % 2 == 0
                ca, cb = slab_range(npts, ldist, l + 1, r, nranks)
                assert a == 2 * ca and b == (n if r == nranks - 1 else 2 * cb)
            prev_end = b
        assert prev_end == n


@pytest.mark.parametrize("npts,levels", [(9, 2), (17, 3), (33, 4)])
@pytest.mark.parametrize("style", [0, 1, 2])
def test_implicit_maps_equal_the_reference_maps_bit_exactly(npts, levels, style):
    """a9: the product keeps no index arrays; its formula maps must reproduce, entry for entry, the grid->global and
    global->(i,j,g) arrays the reference builds (src/matbuild.c:146-323, restated in the oracle) for every -map style
    when each level holds one grid, and its ranges for any number of ranks.  The same against the arrays the reference itself computed
    (tests/golden/ref_maps.npz, recorded by oracle/ref_record.c): the oracle is a restatement, the recording is not."""
    import ctypes as C
    import ref_fixtures as RF
    from multigrid_petsc_amd import solver as S
    from oracle import Oracle
    orc = Oracle()
    L = S._lib()
    recorded = RF.load_maps()[0]
    for l in range(levels):
        n = L.mg_grid_n(npts, l)
        tot = n * n
        for procs in (1, 3, 8):
            glob = np.zeros(3 * tot, dtype=np.int32)
            grid = np.zeros(tot, dtype=np.int32)
            ranges = np.zeros(procs + 1, dtype=np.int32)
            assert orc.L.mgo_mapping_2d(npts, levels, levels, style, procs, l, glob.ctypes.data, grid.ctypes.data, ranges.ctypes.data) == 0
            mine = np.array([L.mg_grid_to_global(2, n, 0, i, j) for i in range(n) for j in range(n)], dtype=np.int64)
            assert np.array_equal(mine, grid)
            k, i, j = C.c_int(), C.c_int(), C.c_int()
            for idx in range(tot):
                L.mg_global_to_grid(2, n, idx, C.byref(k), C.byref(i), C.byref(j))
                assert (i.value, j.value, l) == tuple(glob[3 * idx:3 * idx + 3])
            assert np.array_equal(S.get_ranges(tot, procs), ranges)
        for procs in (1, 2, 3, 4, 8):
            rec = recorded[(npts, levels, levels, style, procs)]
            assert int(rec["grids"][l]) == 1 and int(rec["total"][l]) == tot and rec["grid"][l][0].shape == (n, n)     # mg_grid_n
            mine = np.array([L.mg_grid_to_global(2, n, 0, i, j) for i in range(n) for j in range(n)], dtype=np.int32)
            assert RF.same_bits(mine, rec["grid"][l][0].reshape(-1))
            back = np.zeros((tot, 3), dtype=np.int32)
            k, i, j = C.c_int(), C.c_int(), C.c_int()
            for idx in range(tot):
                L.mg_global_to_grid(2, n, idx, C.byref(k), C.byref(i), C.byref(j))
                back[idx] = (i.value, j.value, l)
            assert RF.same_bits(back, rec["glob"][l])
            assert RF.same_bits(np.asarray(S.get_ranges(tot, procs), dtype=np.int32), rec["ranges"][l])


def test_teeth_of_the_recorded_map_comparison():
    """the helper the comparison above uses reports two swapped map entries and a ranges entry off by one"""
    import ref_fixtures as RF
    rec = RF.load_maps()[0][(17, 3, 3, 1, 3)]
    grid, ranges = rec["grid"][0][0].reshape(-1), rec["ranges"][0]
    assert RF.same_bits(grid.copy(), grid) and RF.same_bits(ranges.copy(), ranges)
    swapped = grid.copy()
    swapped[[17, 18]] = swapped[[18, 17]]
    off = ranges.copy()
    off[1] += 1
    assert not RF.same_bits(swapped, grid) and not RF.same_bits(off, ranges)


def _petsc_surface():
    """every function include/petscksp.h declares (prototypes only: `type name(args);` at the start of a line)"""
    txt = open(os.path.join(ROOT, "include", "petscksp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = "\n".join(l for l in txt.splitlines() if not l.lstrip().startswith("#"))
    names = re.findall(r"^\s*(?:PetscErrorCode|PetscViewer|int|double)\s+([A-Za-z_][A-Za-z0-9_]*)\s*\(", txt, flags=re.M)
    return sorted(set(names))


def test_libmgpetsc_exports_the_whole_petsc_surface():
    """the drop-in must export every PETSc / MPI entry point its header promises the reference driver"""
    from multigrid_petsc_amd._lib import load_mgpetsc
    L = load_mgpetsc()
    names = _petsc_surface()
    assert len(names) >= 80 and "KSPSolve" in names and "MPI_Wtime" in names and "PCMGSetX" in names
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, f"libmgpetsc.so does not export {missing}"


def test_reference_objects_need_nothing_the_drop_in_lacks():
    """The reference's six UNMODIFIED sources, compiled against include/petscksp.h by __graft_entry__.build() where the reference
    is present (oracle/Makefile `ref`: oracle/_ref/o1): every undefined symbol of the objects must be exported by libmgpetsc.so /
    libmgk.so or come from libc / libm -- the link of oracle/_ref/poisson cannot fail on a missing PETSc entry point."""
    import subprocess
    objs = [os.path.join(ROOT, "oracle", "_ref", "o1", f + ".o") for f in ("array", "matbuild", "mesh", "problem", "solver", "poisson")]
    if not all(os.path.exists(o) for o in objs):
        pytest.skip("oracle/_ref/o1 is not built (no reference tree at build time)")
    from multigrid_petsc_amd._lib import load_mgpetsc, load_mgk
    Lp, Lk = load_mgpetsc(), load_mgk()
    libc = C.CDLL(None)
    libm = C.CDLL("libm.so.6")
    undefined = set()
    for o in objs:
        out = subprocess.run(["nm", "-u", o], check=True, stdout=subprocess.PIPE, text=True).stdout
        undefined |= {l.split()[-1] for l in out.splitlines() if l.strip()}
    defined = set()
    for o in objs:
        out = subprocess.run(["nm", "--defined-only", o], check=True, stdout=subprocess.PIPE, text=True).stdout
        defined |= {l.split()[-1] for l in out.splitlines() if l.strip()}
    need = sorted(undefined - defined - {"_GLOBAL_OFFSET_TABLE_"})
    surface = set(_petsc_surface())
    missing = [n for n in need if not (hasattr(Lp, n) or hasattr(Lk, n) or hasattr(libc, n) or hasattr(libm, n))]
    assert not missing, f"undefined in the reference objects and provided by nobody: {missing}"
    petsc_like = [n for n in need if re.match(r"(Petsc|Vec|Mat|KSP|PC|IS|MPI_|PETSC_)", n)]
    assert len(petsc_like) >= 60
    not_declared = [n for n in petsc_like if n not in surface]
    assert not not_declared, f"used by the reference but not declared in include/petscksp.h: {not_declared}"


def test_own_driver_refuses_option_combinations_it_does_not_build(tmp_path):
    """mgpoisson checks its options before it touches the GPU: -grids != -levels (several grids per level), -map outside 0..2,
    another -pc_type or -cycle stop with exit code 2 and a message (the reference guards its own combinations the same way,
    src/poisson.c:61-71)"""
    import subprocess
    exe = os.path.join(ROOT, "multigrid_petsc_amd", "mgpoisson")
    if not os.path.exists(exe):
        pytest.skip("mgpoisson is not built")
    for args, msg in ((["-levels", "2", "-grids", "3"], "-grids 3 differs from -levels 2"), (["-map", "5"], "-map must be"),
                      (["-pc_type", "ilu"], "only -pc_type jacobi"), (["-cycle", "3"], "only -cycle 0")):
        p = subprocess.run([exe] + args, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert p.returncode == 2 and msg in p.stdout, (args, p.returncode, p.stdout)


# mg_fuse_bits (include/mgsolve.h): the values are ABI -- tests, bench.py, the tools and `mgpoisson -mg_fuse N` pass numerals
FUSE_BITS = {"RESNORM": 1, "PROLONG_SWEEP": 2, "RES_RESTRICT": 4, "NORM_SWEEP": 8, "MIXED_CORRECT": 16, "PAIRS": 32, "RES_RESTRICT_SMALL": 128,
             "COARSE_ZERO_SWEEP": 256, "LDS_TAIL": 512, "SWEEP_RESTRICT": 1024, "ZERO_TRIPLE": 2048, "PROLONG_PAIR": 4096, "TRIPLE_2D": 8192,
             "PROLONG_PAIR_SLAB": 16384, "CHEBY": 32768}
FUSE_DEFAULT = 63 | 256 | 512 | 1024 | 2048 | 4096 | 8192 | 16384 | 32768      # what mg_solver_create has always made of fuse = -1


def _cc(args):
    import shutil
    import subprocess
    if shutil.which(args[0]) is None:
        pytest.skip("no host compiler")
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, " ".join(args) + "\n" + p.stdout[-3000:]


def test_fuse_bit_names_of_the_header_and_of_the_python_mirror(tmp_path):
    """every MG_FUSE_* enumerator of include/mgsolve.h, as a C compiler evaluates it, equals the member of multigrid_petsc_amd.Fuse of that
    name; the named bits are the distinct powers of two they have always been, and MG_FUSE_DEFAULT is the mask fuse = -1 has always selected"""
    import subprocess
    from multigrid_petsc_amd import Fuse
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgsolve.h")).read(), flags=re.S)
    names = re.findall(r"\bMG_FUSE_([A-Z0-9_]+)\s*=", re.search(r"typedef enum mg_fuse_bits \{(.*?)\}", txt, flags=re.S).group(1))
    assert len(names) == len(set(names)) and set(names) == set(FUSE_BITS) | {"DEFAULT"}
    (tmp_path / "fuse.c").write_text('#include <stdio.h>\n#include "mgsolve.h"\nint main(void) {\n'
                                     + "".join(f'    printf("{n} %d\\n", (int)MG_FUSE_{n});\n' for n in names) + "    return 0;\n}\n")
    _cc(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "fuse.c"), "-o", str(tmp_path / "fuse")])
    out = subprocess.run([str(tmp_path / "fuse")], check=True, stdout=subprocess.PIPE, text=True).stdout
    header = {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}
    assert header == {n: int(m) for n, m in Fuse.__members__.items()}
    bits = {n: v for n, v in header.items() if n != "DEFAULT"}
    assert bits == FUSE_BITS
    assert all(v > 0 and v & (v - 1) == 0 for v in bits.values()) and len(set(bits.values())) == len(bits)
    assert header["DEFAULT"] == FUSE_DEFAULT == int(Fuse.DEFAULT)
    assert not header["DEFAULT"] & (64 | FUSE_BITS["RES_RESTRICT_SMALL"])          # (64 is unassigned, bit 7 is for tests)


def test_tuning_names_of_the_header_and_of_the_python_mirror(tmp_path):
    """every MGK_TUNE_* enumerator of include/mgk.h, as a C compiler evaluates it, equals the member of multigrid_petsc_amd.Tune of that name
    (aliases included); the forms from 30 up are distinct values, and 57 stays reserved"""
    import subprocess
    from multigrid_petsc_amd import Tune
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgk.h")).read(), flags=re.S)
    names = re.findall(r"\bMGK_TUNE_([A-Z0-9_]+)\s*=", re.search(r"enum mgk_tune \{(.*?)\}", txt, flags=re.S).group(1))
    assert len(names) == len(set(names)) and len(names) >= 30
    (tmp_path / "tune.c").write_text('#include <stdio.h>\n#include "mgk.h"\nint main(void) {\n'
                                     + "".join(f'    printf("{n} %d\\n", (int)MGK_TUNE_{n});\n' for n in names) + "    return 0;\n}\n")
    _cc(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "tune.c"), "-o", str(tmp_path / "tune")])
    out = subprocess.run([str(tmp_path / "tune")], check=True, stdout=subprocess.PIPE, text=True).stdout
    header = {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}
    assert header == {n: int(m) for n, m in Tune.__members__.items()}
    forms = [v for v in header.values() if v >= 30]
    assert len(forms) == len(set(forms)) and header["DEFAULT"] == -1 and header["RESERVED_57"] == 57
    assert (header["STORE_PLAIN"], header["STORE_NT"]) == (0, 1)


def test_fuse_default_by_name_runs_the_cycle_of_minus_one(tmp_path):
    """the own driver over tests/mock_mgk.cpp (csrc/mg_solver.c + mg_comm.c, as tests/test_host_sanitized.py links it), 2-D npts 33, 4 levels,
    two cycles: -mg_fuse <Fuse.DEFAULT> and -mg_fuse -1 take the same passes and leave the same residual history and the same field, digit for
    digit (%.16e prints a double exactly)"""
    import subprocess
    from multigrid_petsc_amd import Fuse
    out = os.path.join(ROOT, "tests", "_san")
    os.makedirs(out, exist_ok=True)
    csrc = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
    flags = ["-O1", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L", "-I" + os.path.join(ROOT, "include")]
    mock = os.path.join(out, "abi_mock_mgk.o")
    _cc(["g++", "-std=c++17"] + flags + ["-c", os.path.join(ROOT, "tests", "mock_mgk.cpp"), "-o", mock])
    exe = os.path.join(out, "abi_mgpoisson")
    _cc(["gcc", "-std=c99"] + flags + [os.path.join(csrc, "driver", "mgpoisson.c"), os.path.join(csrc, "mg_solver.c"), os.path.join(csrc, "mg_comm.c"), mock,
                                      "-o", exe, "-lstdc++", "-lm", "-ldl", "-lpthread"])
    res = {}
    for fuse in (-1, int(Fuse.DEFAULT), 0):
        d = tmp_path / f"fuse{fuse}"
        d.mkdir()
        p = subprocess.run([exe, "-dim", "2", "-npts", "33", "-levels", "4", "-iter", "2", "-ksp_richardson_scale", "0.8", "-pc_type", "jacobi", "-mg_fuse", str(fuse),
                            "-write_fields", "1"], cwd=d, env=dict(os.environ, MOCK_MGK_STATS="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert p.returncode == 0 and "Number of iterations:\t\t2" in p.stdout, p.stdout[-2000:]
        res[fuse] = ((d / "rData.dat").read_text(), (d / "uData.dat").read_text(), re.findall(r"MOCK_MGK_STATS.*", p.stdout))
    assert len(res[-1][0].split()) == 3 and len(res[-1][1].split()) == 31 * 31
    assert res[int(Fuse.DEFAULT)] == res[-1]
    assert res[0][1] == res[-1][1]                  # (every mask computes the same field: the bits choose passes, not arithmetic)
