"""x-line Jacobi and alternating line relaxation, CPU tier.  The product's mg_solver.c + mg_comm.c + mg_line.c + mg_xline.c over host-memory
stand-ins for the line kernels (tests/mock_mgk_xline.cpp, which includes tests/mock_mgk_line.cpp textually), driven through
Solver(pc_type="xline" | "altline") against tests/xline_reference.py:

  solves        the same count (every case's stop decision is clear of rounding), the history within 1e-12 of rnorm[0], u bit for bit; the
                pinned counts; graph=0 and fuse=0 give the bits of the defaults; reset + solve repeats them
  order         the log of executed line passes is the reference's log of sweeps: y for even, x for odd sweeps of every smoothing, on the
                coarsest level and under v = (2, 1), (1, 2) as well
  tables        mg_xline.c's table against the reference's, bit for bit, meshes 0 / 1 / 2, n = 1 included; stride 0 on the uniform mesh
  as before     yline and jacobi solves on the same build against tests/line_reference.py and the oracle; a library linked without
                mg_xline.c (the y-line tier's link) still links, runs yline and refuses the new smoothers with a message
  sanitizers    the same sources as a plain executable under -fsanitize=address,undefined, refusals and leaks included
  the point     the reference's alternating cycle takes at most 8 cycles at every listed size and mesh, where the y-line cycle takes 18 at
                (129, mesh 2)"""
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
from row_tables import _rt_apply, _rt_tables
from xline_mock_worker import TABLE_LEVELS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
KERNELS = ("mgk_xline_forward_f64", "mgk_xline_backward_f64")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SAN_CASES = [XR.CASES[1], XR.CASES[9], XR.CASES[13], XR.CASES[17]]      # altline mesh 1 and mesh 2 (rough), xline mesh 0 and mesh 1 (rough)
IDS = [XR.xcase_key(c) for c in XR.CASES]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _compile(tag, extra, sources):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src in sources:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"xline_{tag}_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + extra + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    return out, objs


def _sources(mock="mock_mgk_xline.cpp", xline=True):
    return [os.path.join(HERE, mock), os.path.join(CSRC, "mg_solver.c"), os.path.join(CSRC, "mg_comm.c"), os.path.join(CSRC, "mg_line.c")] + \
           ([os.path.join(CSRC, "mg_xline.c")] if xline else [])


def _link(out, objs, name):
    so = os.path.join(out, name)
    p = subprocess.run(["g++", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return so


@pytest.fixture(scope="module")
def results(orc, tmp_path_factory):
    """every case through Solver in one worker process (the loader caches its libraries)"""
    out, objs = _compile("plain", [], _sources())
    so = _link(out, objs, "libmgsolve_xline_mock.so")
    npz = str(tmp_path_factory.mktemp("xline") / "res.npz")
    np.savez(npz + ".rows.npz", **{f"tab:{npts},{l},{mesh}": LR.level_table(orc, npts, l, mesh) for npts, l, mesh in TABLE_LEVELS})
    p = subprocess.run([sys.executable, os.path.join(HERE, "xline_mock_worker.py"), so, npz] + IDS,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(npz)


def _letters(log):
    """the reference's log of sweeps as the stand-ins' log of passes: a y sweep is f b, an x sweep F B"""
    return "".join("fb" if kind == "y" else "FB" for _, kind in log)


@pytest.mark.parametrize("case", XR.CASES, ids=IDS)
def test_solve_over_the_mock_equals_the_reference(orc, results, case):
    k = XR.xcase_key(case) + ":"
    ref = XR.reference(orc, case)
    assert ref["iters"] == case[5], (ref["iters"], case[5])                     # the pinned count is the reference's own
    it = int(results[k + "it"])
    XR.compare(ref, it, results[k + "rn"], results[k + "u"], float(results[k + "bnorm"]))
    assert str(results[k + "log"]) == _letters(ref["log"])
    levels, n0 = case[2], case[1] - 2
    assert float(results[k + "dof"]) == sum((3 if l == levels - 1 else 6) * float((case[1] - 1) // 2 ** l - 1) ** 2 for l in range(levels)), n0
    for tag in ("graph0", "fuse0"):
        assert int(results[k + tag + "_it"]) == it
        assert np.array_equal(results[k + tag + "_rn"], results[k + "rn"]) and np.array_equal(results[k + tag + "_u"], results[k + "u"]), tag


@pytest.mark.parametrize("v", [(2, 1), (3, 3), (1, 2)])
def test_every_smoothing_starts_with_a_y_sweep(orc, results, v):
    """17, 4 levels, mesh 1, altline: per cycle v0 sweeps y x y .. on every level going down, v1 on the coarsest, v0 going up -- each
    smoothing counted from 0, so each starts with y; with and without the recorded graph; and the reference's solution"""
    h = XR.Hierarchy(orc, 17, 4, 1, "altline")
    ref = XR.solve(h, h.rhs(), XR.SCALE, v=v, rtol=XR.RTOL, maxiter=100)
    one = lambda k: "".join("fb" if q % 2 == 0 else "FB" for q in range(k))
    cycle = one(v[0]) * 3 + one(v[1]) + one(v[0]) * 3
    for graph in (1, 0):
        k = f"order:{v[0]},{v[1]},{graph}:"
        assert int(results[k + "it"]) == ref["iters"]
        assert str(results[k + "log"]) == cycle * ref["iters"] == _letters(h.log), (v, graph)
        assert np.array_equal(results[k + "u"], ref["u"])
        assert np.abs(results[k + "rn"] - ref["rnorm"]).max() <= 1e-12 * ref["rnorm"][0]


def test_x_tables_bit_for_bit(orc, results):
    for npts, l, mesh in TABLE_LEVELS:
        ct = LR.level_table(orc, npts, l, mesh)
        n = ct.shape[0]
        want = XR.table(ct)
        got = results[f"tab:{npts},{l},{mesh}"]
        if mesh == 0:
            assert got.shape == (1, n) and all(np.array_equal(got[0], want[i]) for i in range(n)), (npts, l)      # one row serves every row
        else:
            assert np.array_equal(got[:, :n], want) and not got[:, n:].any(), (npts, l, mesh)                     # the padding is zero
    assert any(LR.level_table(orc, npts, l, mesh).shape[0] == 1 for npts, l, mesh in TABLE_LEVELS if mesh)


def test_yline_and_jacobi_are_what_they_were(orc, results):
    """the same build: yline against tests/line_reference.py, jacobi against the oracle's cycle"""
    for npts, levels, mesh in ((65, 6, 1), (17, 4, 2)):
        k = f"old:yline,{npts},{levels},{mesh}:"
        h = LR.Hierarchy(orc, npts, levels, mesh)
        ref = LR.solve(h, h.rhs(), LR.SCALE)
        assert int(results[k + "it"]) == ref["iters"] and np.array_equal(results[k + "u"], ref["u"])
        assert np.abs(results[k + "rn"] - ref["rnorm"]).max() <= 1e-12 * ref["rnorm"][0]
    for npts, levels, mesh in ((33, 5, 0), (33, 5, 1)):
        k = f"old:jacobi,{npts},{levels},{mesh}:"
        ref = orc.vcycle(2, npts, levels, 3, 3, maxiter=100, scale=LR.SCALE, use_csr=1 if mesh else 0, mesh=mesh)
        assert int(results[k + "it"]) == ref["iters"] and np.array_equal(results[k + "u"], ref["u"])
        assert np.abs(results[k + "rn"] - ref["rnorm"]).max() <= 1e-12 * ref["rnorm"][0]


def test_a_library_without_mg_xline_links_and_refuses(orc, tmp_path):
    """the y-line tier's link (mock_mgk_line.cpp + mg_solver.c + mg_comm.c + mg_line.c): no strong reference to anything new"""
    out, objs = _compile("noxline", [], _sources("mock_mgk_line.cpp", xline=False))
    so = _link(out, objs, "libmgsolve_noxline_mock.so")
    lib = ctypes.CDLL(so)
    assert not hasattr(lib, "mg_xline_smooth") and hasattr(lib, "mg_line_smooth")
    npz = str(tmp_path / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "xline_mock_worker.py"), so, npz, "--without-mg-xline"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    r = np.load(npz)
    h = LR.Hierarchy(orc, 17, 4, 1)
    ref = LR.solve(h, h.rhs(), LR.SCALE)
    assert int(r["it"]) == ref["iters"] == 9 and np.array_equal(r["u"], ref["u"])


@pytest.fixture(scope="module")
def san_exe():
    """the same sources as one executable with -fsanitize=address,undefined, built once"""
    out, objs = _compile("san", SAN, _sources() + [os.path.join(HERE, "san_xline.c")])
    exe = os.path.join(out, "san_xline")
    p = subprocess.run(["g++"] + SAN + ["-o", exe] + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("case", SAN_CASES, ids=[XR.xcase_key(c) for c in SAN_CASES])
def test_solve_under_sanitizers(orc, san_exe, tmp_path, case):
    """under -fsanitize=address,undefined: no report (leaks included: every table is freed by mg_solver_destroy, a refused creation leaves
    nothing), the refusals, and results that pass the same bars"""
    pc, npts, levels, mesh, rhs = case[:5]
    ref = XR.reference(orc, case)
    rhsfile = "-"
    if rhs != "manufactured":
        import rhs_cases
        rhsfile = str(tmp_path / "rhs.bin")
        rhs_cases.uniform(2, npts, int(rhs.split(":")[1])).tofile(rhsfile)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    txt = str(tmp_path / "out.txt")
    p = subprocess.run([san_exe, {"xline": "2", "altline": "3"}[pc], str(npts), str(levels), str(mesh), repr(XR.SCALE), rhsfile, txt], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:]
    got = {ln.split(" ", 1)[0]: ln.split()[1:] for ln in open(txt)}
    for tag in ("solve", "again"):
        rn = np.array(got[tag + "_rnorm"], dtype=float)
        XR.compare(ref, int(got[tag + "_iters"][0]), rn, np.array(got[tag + "_u"], dtype=float), ref["bnorm"])


def test_alternating_counts_do_not_grow_with_the_size(orc):
    """what the feature is for: the reference's alternating cycle takes at most 8 cycles on every listed size and mesh, and its iterate is
    converged; the y-line cycle takes 18 at (129, mesh 2)"""
    for case in XR.CASES:
        if case[0] != "altline":
            continue
        ref = XR.reference(orc, case)
        assert ref["iters"] == case[5] <= 8, case
    npts, mesh = 129, 2
    assert XR.reference(orc, ("altline", npts, 7, mesh, "rough:1", 7))["iters"] == 7
    h = LR.Hierarchy(orc, npts, 7, mesh)
    b = h.rhs()
    assert LR.solve(h, b, LR.SCALE)["iters"] == 18
    a = XR.Hierarchy(orc, npts, 7, mesh, "altline")
    r = XR.solve(a, b, XR.SCALE)
    n = npts - 2
    res = b.reshape(n, n) - _rt_apply(a.ct[0], r["u"].reshape(n, n))
    assert r["iters"] <= 8 and np.sqrt(np.sum(res * res)) <= XR.RTOL * r["bnorm"]


def test_an_x_sweep_solves_the_x_tridiagonal_part(orc):
    """the table factorises T_x: after one sweep with scale 1 from the zero guess T_x u = b to rounding, on random row tables with W != E
    and on stretched levels; and the x sweep is the y sweep of the transposed problem where the rows are constant (the uniform mesh)"""
    rng = np.random.default_rng(6)
    from coef_cases import distinct_row_tables
    for ct in (distinct_row_tables(rng, 31)[0], _rt_tables(rng, 17)[0], LR.level_table(orc, 65, 0, 1), LR.level_table(orc, 33, 1, 2)):
        n = ct.shape[0]
        if abs(ct[:, 2]).min() <= (abs(ct[:, 1]) + abs(ct[:, 3])).max():
            ct = ct.copy()
            ct[:, 2] = 3.0 * (abs(ct[:, 1]) + abs(ct[:, 3]))            # make T_x diagonally dominant: the statement is about the factorisation
        b = rng.uniform(-1, 1, (n, n))
        u = XR.sweep(ct, XR.table(ct), 1.0, b)
        tx = ct.copy()
        tx[:, 0] = 0.0
        tx[:, 4] = 0.0                                   # T_x: the W, C, E entries alone
        assert np.abs(_rt_apply(tx, u) - b).max() <= 1e-12 * np.abs(b).max()
    ct = LR.level_table(orc, 33, 0, 0)
    n = ct.shape[0]
    ct = np.tile(ct[1], (n, 1))                          # the five constants in every row (the assembled edge rows drop S / N)
    b, u = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    cy = ct[:, [1, 0, 2, 4, 3]]                          # the transposed operator: S <-> W, N <-> E
    ux = XR.sweep(ct, XR.table(ct), 0.8, b, u)
    uy = LR.sweep(cy, LR.tables(cy), 0.8, b.T.copy(), u.T.copy()).T
    assert np.abs(ux - uy).max() <= 1e-13


def test_the_entry_points_are_built_and_only_mg_xline_names_the_kernels():
    """the two kernels are declared and exported by libmgk.so, the hooks by libmgpetsc.so; of the host sources only mg_xline.c names the
    kernels, and neither mg_solver.c nor mg_line.c names anything of mg_xline.c outside the weak references"""
    hk, hs = open(os.path.join(ROOT, "include", "mgk.h")).read(), open(os.path.join(ROOT, "include", "mgsolve.h")).read()
    assert all(k + "(" in hk for k in KERNELS) and "MG_PC_LINE_X = 2" in hs and "MG_PC_LINE_ALT = 3" in hs
    lib = os.path.join(ROOT, "multigrid_petsc_amd")
    Lk = ctypes.CDLL(os.path.join(lib, "libmgk.so"))
    Lp = ctypes.CDLL(os.path.join(lib, "libmgpetsc.so"))
    assert all(hasattr(Lk, k) for k in KERNELS)
    assert hasattr(Lp, "mg_xline_smooth") and hasattr(Lp, "mg_xline_tables")
    for f in ("mg_solver.c", "mg_line.c", "mg_comm.c", "mg_fmg.c", "mg_gmres.c", "mg_cheby.c", "petsc_shim.c", os.path.join("driver", "mgpoisson.c")):
        text = open(os.path.join(CSRC, f)).read()
        for name in KERNELS:
            assert name not in text, f"{f} names {name}"
    assert "mg_xline" not in open(os.path.join(CSRC, "mg_line.c")).read()
    text = open(os.path.join(CSRC, "mg_xline.c")).read()
    assert all(k + "(" in text for k in KERNELS)
    from multigrid_petsc_amd.solver import _PC
    assert _PC == {"jacobi": 0, "yline": 1, "xline": 2, "altline": 3}


def test_own_driver_takes_pc_type_altline(tmp_path):
    """mgpoisson: -pc_type altline is accepted (the run then stops where it needs a GPU or finishes), what it does not know stops with
    exit code 2 and a message that names altline"""
    exe = os.path.join(ROOT, "multigrid_petsc_amd", "mgpoisson")
    assert os.path.exists(exe), "mgpoisson is not built (csrc/Makefile builds it with the libraries)"
    p = subprocess.run([exe, "-pc_type", "zebra"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 2 and "-pc_type altline" in p.stdout, (p.returncode, p.stdout)
    src = open(os.path.join(CSRC, "driver", "mgpoisson.c")).read()
    assert '"altline")) c.pc_type = MG_PC_LINE_ALT' in src
