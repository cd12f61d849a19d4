"""The oracle and the product's host arithmetic against RECORDED REFERENCE OUTPUT (tests/golden/ref_maps.npz, ref_assembly.npz: what the
reference's own matbuild.c / mesh.c / problem.c / solver.c computed and handed to PETSc before a solve, recorded by oracle/ref_record.c over
the reference's unmodified objects; tests/ref_fixtures.py holds the case lists and the views).  CPU tier, every comparison bit for bit:

  freshness   where oracle/_ref/record exists the committed arrays are reproduced
  oracle      maps, ranges, grid ids, sizes, h and the transfer stencils; A / R / P as CSR with their sparsity pattern; b[0]; coordinates;
              mesh.h; GetError on a fixed field
  goldens     the ranges_n*_p* of vcycle_golden.npz (made by a Python formula) against the recorded ranges
  product     tests/ref_tables_dump.c (mg_solver.c's coefficient tables and right-hand side over the host stand-ins of the kernel ABI), plain
              and under -fsanitize=address,undefined as a stand-alone executable
  teeth       a copy of the recorded data with ONE change (a value moved by one ulp, two map entries swapped, a ranges entry off by one) is
              reported unequal by the helpers the comparisons use

The drop-in fed with the recorded call stream is tests/shim_semantics.py: reference_streams (tests/test_shim_semantics_cpu.py); the product's
map formulas against the recorded maps are in tests/test_abi.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_fixtures as RF
from oracle import Oracle, _p

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ONE_GRID = [c for c in RF.ASSEMBLY_CASES if RF.one_grid_per_level(c)]
RHS_ONLY = [c for c in RF.ASSEMBLY_CASES if not c[5]]
COUNT = {"n": 0}


def eq(got, want, what):
    """THE comparison of this file: same shape, same type, same bits"""
    COUNT["n"] += 1
    got, want = np.asarray(got), np.asarray(want)
    if not RF.same_bits(got, want):
        bad = np.nonzero(np.ravel(got != want))[0] if got.shape == want.shape else []
        first = (int(bad[0]), np.ravel(got)[bad[0]], np.ravel(want)[bad[0]]) if len(bad) else (got.shape, want.shape, got.dtype, want.dtype)
        raise AssertionError((what, "first difference (index, got, want)", first))


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def maps():
    return RF.load_maps()


@pytest.fixture(scope="module")
def asm():
    yield RF.load_assembly()
    print(f"\n[reference fixtures, CPU tier: {COUNT['n']} bit-exact comparisons]")


# ---------------------------------------------------------------- freshness
def test_committed_fixtures_are_what_the_recorder_gives():
    """rerun every case and require the committed arrays bit for bit (reads oracle/_ref/record and tests/golden only)"""
    if not os.path.exists(RF.RECORD):
        pytest.skip("oracle/_ref/record is not built (no reference tree at build time)")
    for path, fresh in ((RF.MAPS_NPZ, RF.build_maps()), (RF.ASSEMBLY_NPZ, RF.build_assembly())):
        have = np.load(path, allow_pickle=False)
        assert sorted(have.files) == sorted(fresh)
        for k in have.files:
            eq(have[k], fresh[k], (os.path.basename(path), k))
    assert os.path.getsize(RF.MAPS_NPZ) < 1000000 and os.path.getsize(RF.ASSEMBLY_NPZ) < 1000000


def test_fixture_files_hold_numbers_only():
    for path in (RF.MAPS_NPZ, RF.ASSEMBLY_NPZ):
        z = np.load(path, allow_pickle=False)
        assert all(z[k].dtype in (np.int32, np.float64) for k in z.files)
    assert set(RF.load_maps()[0]) == set(RF.MAP_CASES) and set(RF.load_assembly()) == set(RF.ASSEMBLY_CASES)


# ---------------------------------------------------------------- oracle, integers
def _oracle_maps(orc, case):
    """the oracle's statement of one maps case, in the shape of ref_fixtures.load_maps' entries"""
    npts, grids, levels, style, procs = case
    ng = np.zeros(levels, dtype=np.int32)
    ids = np.zeros(grids, dtype=np.int32)
    assert orc.L.mgo_grid_ids(grids, levels, _p(ng), _p(ids)) == grids
    out = {"grids": ng, "gridid": ids, "total": np.array([orc.L.mgo_level_total_2d(npts, grids, levels, l) for l in range(levels)], dtype=np.int32),
           "h": np.array([[orc.level_stencil(2, npts, int(g))[1]] * 2 for g in ids]), "ranges": np.zeros((levels, procs + 1), dtype=np.int32),
           "glob": [], "grid": []}
    q = 0
    for l in range(levels):
        tot = int(out["total"][l])
        glob, grid, rg = np.zeros(3 * tot, dtype=np.int32), np.zeros(tot, dtype=np.int32), np.zeros(procs + 1, dtype=np.int32)
        assert orc.L.mgo_mapping_2d(npts, grids, levels, style, procs, l, _p(glob), _p(grid), _p(rg)) == 0
        out["ranges"][l] = rg
        out["glob"].append(glob.reshape(-1, 3))
        per, o = [], 0
        for _ in range(int(ng[l])):
            n = orc.L.mgo_grid_n(npts, int(ids[q]))
            per.append(grid[o:o + n * n].reshape(n, n))
            o += n * n
            q += 1
        assert o == tot
        out["grid"].append(per)
    return out


def _eq_maps(got, want, case):
    for k in ("grids", "gridid", "total", "h", "ranges"):
        eq(got[k], want[k], (case, k))
    for l in range(len(want["glob"])):
        eq(got["glob"][l], want["glob"][l], (case, "global -> (i, j, g)", l))
        assert len(got["grid"][l]) == len(want["grid"][l])
        for lg, (a, b) in enumerate(zip(got["grid"][l], want["grid"][l])):
            eq(a, b, (case, "grid -> global", l, lg))


@pytest.mark.parametrize("shape", RF.MAP_SHAPES, ids=lambda s: "n%d_g%d_l%d" % s)
def test_oracle_maps_ranges_and_sizes_equal_the_recorded_ones(orc, maps, shape):
    """mgo_mapping_2d, mgo_get_ranges, mgo_grid_ids, mgo_grid_n, mgo_level_total_2d and mgo_level_stencil's h against src/matbuild.c's own
    output, -map 0/1/2 at 1/2/3/4/8 ranks, -grids >= -levels.  mgo_get_ranges(total) is the level's ranges where the reference calls
    GetRanges on the level's total: a level of one grid, or -map 0 (src/matbuild.c:306); with several grids -map 1 / 2 split the FINE grid
    and let the coarser points follow (:165, :252) -- those ranges come out of mgo_mapping_2d alone."""
    for style in (0, 1, 2):
        for procs in (1, 2, 3, 4, 8):
            case = shape + (style, procs)
            want = maps[0][case]
            _eq_maps(_oracle_maps(orc, case), want, case)
            for l in range(shape[2]):
                if style != 0 and int(want["grids"][l]) > 1:
                    continue
                rg = np.zeros(procs + 1, dtype=np.int32)
                orc.L.mgo_get_ranges(int(want["total"][l]), procs, _p(rg))
                eq(rg, want["ranges"][l], (case, "mgo_get_ranges", l))


def test_oracle_ranges_of_the_ranges_only_cases(orc, maps):
    for case, want in maps[1].items():
        npts, grids, levels, _, procs = case
        for l in range(levels):
            rg = np.zeros(procs + 1, dtype=np.int32)
            orc.L.mgo_get_ranges(orc.L.mgo_level_total_2d(npts, grids, levels, l), procs, _p(rg))
            eq(rg, want[l], (case, l))


def test_committed_golden_ranges_equal_the_recorded_ranges(maps):
    """vcycle_golden.npz's ranges_n*_p* come from a Python formula (tests/golden/make_golden.py: maps); every one of them has a recorded
    counterpart (the maps list was extended by (9, 3, 3) and (17, 4, 4), ranges only)"""
    gold = np.load(os.path.join(HERE, "golden", "vcycle_golden.npz"))
    keys = [k for k in gold.files if k.startswith("ranges_n")]
    assert len(keys) == 12
    for k in keys:
        npts, procs = (int(v) for v in k[len("ranges_n"):].split("_p"))
        levels = gold[k].shape[0]
        rec = maps[1].get((npts, levels, levels, 2, procs))
        if rec is None:
            rec = maps[0][(npts, levels, levels, 2, procs)]["ranges"]
        eq(gold[k].astype(np.int32), rec, k)


# ---------------------------------------------------------------- oracle, values
def _oracle_csr(orc, m):
    rows = orc.csr_rows(m)
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    out = (rowptr, np.concatenate([c for c, _ in rows]).astype(np.int32), np.concatenate([v for _, v in rows]))
    assert orc.L.mgo_csr_nnz(m) == out[1].size
    nr, nc = orc.L.mgo_csr_nrows(m), orc.L.mgo_csr_ncols(m)
    orc.L.mgo_csr_free(m)
    return out, (nr, nc)


def _eq_csr(got, want, what):
    COUNT["n"] += 1
    assert RF.same_csr(got, want), (what, "rowptr / col / val differ",
                                    [int(np.sum(np.asarray(g) != np.asarray(w))) if len(g) == len(w) else (len(g), len(w)) for g, w in zip(got, want)])


def _totals(npts, levels):
    return [((npts - 1) // 2 ** l - 1) ** 2 for l in range(levels)]


@pytest.mark.parametrize("case", ONE_GRID, ids=lambda c: "mesh%d_n%d_l%d" % (c[0], c[1], c[3]))
def test_oracle_matrices_equal_the_recorded_stream(orc, asm, case):
    """mgo_build_A / _A_mesh / _R / _P against the reference's MatSetValue stream reduced to CSR (ADD_VALUES duplicates summed in call order,
    columns ascending): values AND sparsity pattern"""
    mesh, npts, _, levels, _, _ = case
    c = asm[case]
    tot = _totals(npts, levels)
    for l in range(levels):
        want = RF.stream_csr(c, RF.KIND_A, l, tot[l])
        got, shape = _oracle_csr(orc, orc.L.mgo_build_A_mesh(npts, l, mesh))
        assert shape == (tot[l], tot[l])
        _eq_csr(got, want, (case, "mgo_build_A_mesh", l))
        if mesh == 0:
            _eq_csr(_oracle_csr(orc, orc.build("A", 2, npts, l))[0], want, (case, "mgo_build_A", l))
        if l < levels - 1:
            for kind, which in ((RF.KIND_R, "R"), (RF.KIND_P, "P")):
                nr = tot[l + 1] if which == "R" else tot[l]
                got, shape = _oracle_csr(orc, orc.build(which, 2, npts, l))
                assert shape == ((tot[l + 1], tot[l]) if which == "R" else (tot[l], tot[l + 1]))
                _eq_csr(got, RF.stream_csr(c, kind, l, nr), (case, "mgo_build_" + which, l))


@pytest.mark.parametrize("case", RF.ASSEMBLY_CASES, ids=lambda c: "mesh%d_n%d_g%d_l%d_m%d" % c[:5])
def test_oracle_rhs_coordinates_spacings_stencils_and_error_norms(orc, asm, case):
    """mgo_rhs(_mesh), mgo_coords_uniform / _mesh, mgo_mesh_h (uniform mesh: the oracle has no stretched form of it), h per grid, the 3 x 3
    transfer stencils and mgo_error_norms(_mesh) on ref_fixtures.U1 -- GetError's three results.  The oracle accumulates in GetError's loop
    order (row-major, one running sum each), so all three match bit for bit and no tolerance is needed.  Where level 0 holds several grids
    (-grids 3 -levels 1) b[0] goes on with the coarser grids' restricted values, which the oracle does not state: its first (npts - 2)^2
    entries are the fine grid's (-map 2, one rank) and are compared."""
    mesh, npts, grids, levels, _, _ = case
    c = asm[case]
    want_b = RF.stream_vector(c, None if levels == 1 and grids > 1 else (npts - 2) ** 2)[:(npts - 2) ** 2]
    eq(orc.rhs_mesh(npts, mesh), want_b, (case, "mgo_rhs_mesh"))
    cx, cy = np.zeros(npts), np.zeros(npts)
    orc.L.mgo_coords_mesh(npts, 0, mesh, _p(cx)); orc.L.mgo_coords_mesh(npts, 1, mesh, _p(cy))
    eq(cx, c["coord"][0], (case, "mgo_coords_mesh x"))
    eq(cy, c["coord"][1], (case, "mgo_coords_mesh y"))
    eq(np.array([[orc.level_stencil(2, npts, g)[1]] * 2 for g in range(grids)]), c["h"], (case, "h"))
    eq(orc.error_norms_mesh(npts, mesh, RF.U1(npts)), c["error"], (case, "mgo_error_norms_mesh"))
    if mesh == 0:
        eq(orc.rhs(2, npts), want_b, (case, "mgo_rhs"))
        eq(orc.coords(npts), c["coord"][0], (case, "mgo_coords_uniform"))
        eq(orc.coords(npts), c["coord"][1], (case, "mgo_coords_uniform y"))
        eq(np.float64(orc.L.mgo_mesh_h(2, npts)), np.float64(c["mesh_h"]), (case, "mgo_mesh_h"))
        eq(orc.error_norms(2, npts, RF.U1(npts)), c["error"], (case, "mgo_error_norms"))
    if grids > 1:
        w = np.zeros(9)
        orc.L.mgo_restriction_stencil(_p(w))
        eq(w.reshape(3, 3), c["res0"], (case, "mgo_restriction_stencil"))
        orc.L.mgo_prolongation_stencil(_p(w))
        eq(w.reshape(3, 3), c["pro0"], (case, "mgo_prolongation_stencil"))


# ---------------------------------------------------------------- product, host arithmetic
def _build_dump(tag, extra):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src in (os.path.join(HERE, "mock_mgk_line.cpp"), os.path.join(CSRC, "mg_solver.c"), os.path.join(CSRC, "mg_comm.c"), os.path.join(CSRC, "mg_line.c"),
                os.path.join(HERE, "ref_tables_dump.c")):
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"refdump_{tag}_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + extra + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    exe = os.path.join(out, f"ref_tables_dump_{tag}")
    p = subprocess.run(["g++"] + extra + ["-o", exe] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.fixture(scope="module")
def dump_exe():
    return _build_dump("plain", [])


@pytest.fixture(scope="module")
def dump_exe_san():
    return _build_dump("san", SAN)


def _run_dump(exe, tmp_path, npts, levels, mesh):
    txt = str(tmp_path / f"dump_{npts}_{levels}_{mesh}.txt")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, str(npts), str(levels), str(mesh), txt], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    got = {}
    for line in open(txt):
        f = line.split()
        vals = np.array([float.fromhex(v) for v in f[(1 if f[0] == "b" else 2):]])
        if f[0] in ("ctab", "dtab", "b"):
            vals = vals[1:]                                   # (the row count comes first)
        got[(f[0],) if f[0] == "b" else (f[0], int(f[1]))] = vals
    return got


def _check_dump(got, c, case):
    """the product's tables against the recorded A[l]: for every level and every grid row i the row {A(i-1), W, C, E, A(i+1)} of the interior
    column j = n / 2 (the entries the matrix has: no A(i-1) in the first grid row, no A(i+1) in the last), 1 / C, and b[0]"""
    mesh, npts, _, levels, _, full = case
    eq(got[("b",)], RF.stream_vector(c, (npts - 2) ** 2), (case, "level 0's b"))
    if not full:
        return
    for l in range(levels):
        n = (npts - 1) // 2 ** l - 1
        assert n >= 3
        rowptr, col, val = RF.stream_csr(c, RF.KIND_A, l, n * n)
        j = n // 2
        tab = got[("ctab", l)].reshape(n, 5) if mesh else np.tile(got[("coef", l)], (n, 1))
        dtab = got[("dtab", l)] if mesh else np.full(n, got[("dinv", l)][0])
        eq(got[("h", l)], c["h"][l][:1], (case, "h", l))
        for i in range(n):
            r = i * n + j
            cols, vals = col[rowptr[r]:rowptr[r + 1]], val[rowptr[r]:rowptr[r + 1]]
            offs = ([-n] if i > 0 else []) + [-1, 0, 1] + ([n] if i < n - 1 else [])
            assert list(cols) == [r + o for o in offs], (case, l, i, cols)
            slots = [{-n: 0, -1: 1, 0: 2, 1: 3, n: 4}[o] for o in offs]
            eq(tab[i, slots], vals, (case, "coefficients of grid row", l, i))
            eq(dtab[i:i + 1], 1.0 / vals[offs.index(0):offs.index(0) + 1], (case, "1 / C of grid row", l, i))


@pytest.mark.parametrize("case", ONE_GRID + RHS_ONLY, ids=lambda c: "mesh%d_n%d_l%d" % (c[0], c[1], c[3]))
def test_product_host_tables_equal_the_recorded_values(asm, dump_exe, tmp_path, case):
    """coords_mesh_y, metrics_mesh, level_row_tables, level_stencil and sin_tables of mg_solver.c (static: reached through mg_solver_create and
    mg_solver_set_rhs_problem) against what the reference handed to MatSetValue / VecSetValue, on meshes 0/1/2; b also at npts 65 / 129"""
    _check_dump(_run_dump(dump_exe, tmp_path, case[1], case[3], case[0]), asm[case], case)


@pytest.mark.parametrize("case", [(1, 33, 4, 4, 2, 1), (2, 17, 3, 3, 2, 1), (0, 9, 2, 2, 2, 1), (2, 65, 1, 1, 2, 0)], ids=lambda c: "mesh%d_n%d_l%d" % (c[0], c[1], c[3]))
def test_product_host_tables_under_sanitizers(asm, dump_exe_san, tmp_path, case):
    """the same program as a stand-alone executable under -fsanitize=address,undefined: no report (leaks included) and the same values"""
    _check_dump(_run_dump(dump_exe_san, tmp_path, case[1], case[3], case[0]), asm[case], case)


# ---------------------------------------------------------------- teeth
def _ulp_up(a, q):
    a = np.array(a, dtype=np.float64, copy=True)
    a.reshape(-1)[q] = np.nextafter(a.reshape(-1)[q], np.inf)
    return a


def test_teeth_one_value_moved_by_one_ulp(orc, asm):
    case = (1, 17, 3, 3, 2, 1)
    c = asm[case]
    want = RF.stream_csr(c, RF.KIND_A, 0, 225)
    got = _oracle_csr(orc, orc.L.mgo_build_A_mesh(17, 0, 1))[0]
    _eq_csr(got, want, "unchanged")
    with pytest.raises(AssertionError):
        _eq_csr(got, (want[0], want[1], _ulp_up(want[2], 517)), "one matrix value moved by one ulp")
    moved = want[1].copy()
    moved[3], moved[4] = moved[4], moved[3]
    with pytest.raises(AssertionError):
        _eq_csr(got, (want[0], moved, want[2]), "two columns of one row swapped")
    b = RF.stream_vector(c, 225)
    with pytest.raises(AssertionError):
        eq(orc.rhs_mesh(17, 1), _ulp_up(b, 100), "one right-hand-side value moved by one ulp")
    with pytest.raises(AssertionError):
        eq(orc.error_norms_mesh(17, 1, RF.U1(17)), _ulp_up(c["error"], 1), "the sum of GetError moved by one ulp")
    changed = dict(c, val=_ulp_up(c["val"], int(np.nonzero(c["obj"] == 0)[0][40])))
    with pytest.raises(AssertionError):
        _eq_csr(got, RF.stream_csr(changed, RF.KIND_A, 0, 225), "one recorded call moved by one ulp")
    # -0.0 against 0.0 and a changed type are differences too
    assert not RF.same_bits(np.array([0.0]), np.array([-0.0])) and not RF.same_bits(np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64))


def test_teeth_two_map_entries_swapped_and_a_ranges_entry_off_by_one(orc, maps):
    import copy
    case = (17, 3, 2, 1, 3)
    got, want = _oracle_maps(orc, case), maps[0][case]
    _eq_maps(got, want, case)
    swapped = copy.deepcopy(want)
    g = swapped["grid"][1][0]
    g[2, 3], g[2, 4] = int(g[2, 4]), int(g[2, 3])
    with pytest.raises(AssertionError):
        _eq_maps(got, swapped, "two grid -> global entries swapped")
    swapped = copy.deepcopy(want)
    gl = swapped["glob"][1]
    gl[[5, 6]] = gl[[6, 5]]
    with pytest.raises(AssertionError):
        _eq_maps(got, swapped, "two global -> grid entries swapped")
    off = copy.deepcopy(want)
    off["ranges"][1, 2] += 1
    with pytest.raises(AssertionError):
        _eq_maps(got, off, "one ranges entry off by one")


def test_teeth_product_dump(asm, dump_exe, tmp_path):
    """the helper of the product comparison reports one coefficient, one 1 / C and one right-hand-side value moved by one ulp"""
    case = (2, 9, 2, 2, 2, 1)
    got = _run_dump(dump_exe, tmp_path, 9, 2, 2)
    _check_dump(got, asm[case], case)
    for key, q in ((("ctab", 1), 7), (("dtab", 0), 3), (("b",), 20), (("h", 1), 0)):
        with pytest.raises(AssertionError):
            _check_dump({**got, key: _ulp_up(got[key], q)}, asm[case], case)
