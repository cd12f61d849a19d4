"""The x-line sweep in chunks (mg_config.xline_chunk), CPU tier.

  (a) the definition itself, tests/xchunkline_reference.py: with c > nx the chunked sweep is xline_reference.sweep bit for bit (signed zeros
      included); for nx in 1 .. 255 and c in {16, 32, 48, 64} on random, non-symmetric and mesh row tables the solve x = T_x^-1 r (scale 1,
      zero guess, and from a guess) lies within 1e-13 max|x| of the plain one (the bound of section 8h)
  (b) the product's host tables (csrc/mg_xline_chunk.c, written out by tests/xchunk_tables_dump.c) against the reference's, bit for bit, on the
      uniform mesh (one row, strides 0) and on the stretched ones; the padding of the tables is zero
  (c) the product's mg_solver.c + mg_comm.c + mg_line.c + mg_xline.c + mg_line_chunk.c + mg_xline_chunk.c over host-memory stand-ins for the
      four passes (tests/mock_mgk_xchunkline.cpp), through Solver(pc_type="xline" / "altline", xline_chunk=c): npts 33, 65, 129, c in {16, 32},
      meshes 0, 1, 2, and altline with line_chunk set as well: the same count, the history within 1e-12 of rnorm[0], u bit for bit
      (line_reference.compare); graph=0 and fuse=0 give the default's bits; reset + solve repeats them; the stand-ins' execution counts show
      four passes per chunked x sweep, two plain ones on a level with n < c, and the y passes as before
  (d) the same sources as a plain executable under -fsanitize=address,undefined, with the refusals and leak checking
  (e) xline_chunk=0 gives the bits of a solver built without the keyword, of the plain reference, and calls none of the four passes
And the symbols, who names the kernels, the field of MgConfig, the refusals of the own driver and of a link without mg_xline_chunk.c.

The right-hand side of a case is the manufactured one where the reference's stop decision is clear of rounding by line_reference's margins
(last norm <= 0.8, the one before >= 1.5 rtol ||b||), else the first rough seed where it is.  x-line smoothing on mesh 1 (stretched in y) at
npts 65 and 129 contracts by 1.67 and 1.3 per cycle: two consecutive norms cannot lie on both sides of those margins (that takes a factor of
1.875), whatever the right-hand side.  These four cases are held to everything else line_reference.compare asserts -- the same count
(the threshold is 6 % and more away, rounding is 1e-12), the history, u bit for bit."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import line_reference as LR
import xchunkline_reference as XC
import xline_reference as XR
from coef_cases import distinct_row_tables
from oracle import Oracle
from row_tables import _rt_tables

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")
KERNELS = ("mgk_xline_chunk_forward_f64", "mgk_xline_chunk_backward_f64", "mgk_xline_chunk_reduce_f64", "mgk_xline_chunk_correct_f64")
HOST = ("mg_solver.c", "mg_comm.c", "mg_line.c", "mg_xline.c", "mg_line_chunk.c", "mg_xline_chunk.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
LEVELS = {33: 5, 65: 6, 129: 7}
# the right-hand side per (pc, npts, mesh): see the docstring
RHS = {("xline", 33, 1): "rough:1", ("xline", 65, 2): "rough:2", ("xline", 129, 2): "rough:31",
       ("altline", 65, 1): "rough:13", ("altline", 129, 1): "rough:34", ("altline", 129, 2): "rough:1"}
UNCLEAR = {("xline", 65, 1), ("xline", 129, 1)}


def _case(pc, npts, mesh):
    return (npts, LEVELS[npts], mesh, RHS.get((pc, npts, mesh), "manufactured"))


# (pc, xc, yc, case)
SOLVES = [(pc, xc, 0, _case(pc, npts, mesh)) for pc in ("xline", "altline") for npts in (33, 65, 129) for mesh in (0, 1, 2) for xc in (16, 32)]
BOTH = [("altline", 16, 8, _case("altline", 65, 2)), ("altline", 32, 16, _case("altline", 129, 0)), ("altline", 16, 16, _case("altline", 33, 1))]
ZERO = [("xline", 0, 0, _case("xline", 33, 2)), ("altline", 0, 0, _case("altline", 65, 0)), ("altline", 0, 8, _case("altline", 65, 2))]
SAN_CASES = [("xline", 16, 0, _case("xline", 65, 0)), ("altline", 32, 0, _case("altline", 65, 2)), ("altline", 16, 8, _case("altline", 33, 1)),
             ("xline", 16, 0, _case("xline", 33, 1))]
SIZES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 100, 255]
PERIODS = [16, 32, 48, 64]
BOUND = 1e-13
MESH_LEVELS = [(65, 0, 0), (65, 0, 1), (129, 1, 2), (129, 0, 2), (257, 0, 0), (257, 0, 1), (33, 0, 2), (17, 3, 1)]


def _key(pc, xc, yc, case):
    return f"{pc};{xc};{yc};{LR.case_key(case)}"


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _distance(ct, c, seed):
    """max |x_chunked - x_plain| / max |x_plain| of x = T_x^-1 r on a random r (scale 1 from the zero guess), and the same from a guess"""
    n = ct.shape[0]
    rng = np.random.default_rng(seed)
    b, u = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    tab, g = XC.tables(ct, c), XR.table(ct)
    worst = 0.0
    for guess in (None, u):
        p, q = XR.sweep(ct, g, 1.0, b, guess), XC.sweep(ct, tab, 1.0, b, guess)
        x = p if guess is None else p - guess
        worst = max(worst, float(np.abs(p - q).max() / np.abs(x).max()))
        if c > n:
            assert np.array_equal(p, q) and np.array_equal(np.signbit(p), np.signbit(q)), (n, c)
    return worst


def test_the_chunked_sweep_is_the_plain_sweep_to_rounding(orc):
    """(a): bit-identical (signed zeros included) when the period exceeds nx; within 1e-13 max|x| otherwise"""
    worst = (0.0, ("none", 0, 0))
    for n in SIZES:
        for c in PERIODS + [256]:
            for name, mk in (("rt", _rt_tables), ("distinct", distinct_row_tables)):
                d = _distance(mk(np.random.default_rng(100 * n + c), n)[0], c, 7 * n + c)
                worst = max(worst, (d, (name, n, c)))
    for npts, level, mesh in MESH_LEVELS:
        ct = LR.level_table(orc, npts, level, mesh)
        for c in PERIODS + [256]:
            d = _distance(ct, c, npts + c)
            worst = max(worst, (d, ("mesh%d" % mesh, ct.shape[0], c)))
    print(f"largest distance from the plain solve: {worst[0]:.2e} of max|x| at {worst[1]}")
    assert worst[0] <= BOUND, worst


def test_the_layout_and_the_stored_zeros():
    """separators, chunks, and the zeros the edge cases rest on: g, v, w in the separator columns, v on chunk 0, w on the last chunk; a
    rectangular level takes its chunks from the number of columns"""
    assert XC.layout(15, 16) == (0, [(0, 15)], [])
    assert XC.layout(16, 16) == (1, [(0, 15), (16, 16)], [15])
    assert XC.layout(65, 16) == (4, [(0, 15), (16, 31), (32, 47), (48, 63), (64, 65)], [15, 31, 47, 63])
    for n, nx, c in ((65, 65, 16), (64, 64, 16), (33, 100, 32), (100, 33, 16)):
        ct = distinct_row_tables(np.random.default_rng(n + c), n)[0]
        t = XC.tables(ct, c, nx)
        K, chunks, seps = XC.layout(nx, c)
        for name in "gvw":
            assert t[name].shape == (n, nx) and np.all(t[name][:, seps] == 0.0) and not np.any(np.signbit(t[name][:, seps]))
        assert np.all(t["v"][:, :c - 1] == 0.0) and np.all(t["w"][:, K * c:] == 0.0)
        assert np.all(t["w"][:, :c - 1] != 0.0) and np.all(t["v"][:, c:min(2 * c - 1, nx)] != 0.0)
        assert t["SL"].shape == (n, K) and np.all(t["sup"][:, -1] == 0.0) and np.all(t["sup"][:, :-1] != 0.0)


def _compile(tag, extra, sources):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src in sources:
        cxx = src.endswith(".cpp")
        o = os.path.join(out, f"xchunkline_{tag}_{os.path.basename(src)}.o")
        p = subprocess.run(["g++" if cxx else "gcc", "-std=c++17" if cxx else "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off",
                            "-D_POSIX_C_SOURCE=200809L"] + extra + inc + ["-c", src, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        objs.append(o)
    return out, objs


def _sources():
    return [os.path.join(HERE, "mock_mgk_xchunkline.cpp")] + [os.path.join(CSRC, f) for f in HOST]


def _link(args, objs):
    p = subprocess.run(["g++"] + args + objs + ["-lm", "-lpthread", "-ldl"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]


@pytest.fixture(scope="module")
def plain_objs():
    return _compile("plain", [], _sources())


def test_host_tables_equal_the_reference(plain_objs, tmp_path):
    """(b): csrc/mg_xline_chunk.c's tables on the product's own row tables, bit for bit; levels with n < c have none"""
    out, objs = plain_objs
    _, dump = _compile("plain", [], [os.path.join(HERE, "xchunk_tables_dump.c")])
    exe = os.path.join(out, "xchunk_tables_dump")
    _link(["-o", exe], objs + dump)
    for npts, levels, mesh, c in ((65, 6, 0, 16), (129, 7, 0, 32), (65, 6, 1, 16), (129, 7, 2, 48), (65, 6, 2, 32), (33, 5, 1, 16), (129, 7, 1, 64), (65, 6, 2, 64)):
        txt = str(tmp_path / f"t_{npts}_{mesh}_{c}.txt")
        p = subprocess.run([exe, str(npts), str(levels), str(mesh), str(c), txt], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:]
        rec = {}
        for ln in open(txt):
            f = ln.split()
            rec[(f[0], int(f[1]))] = f[2:]
        chunked = 0
        for l in range(levels):
            n = (npts - 1) // (1 << l) - 1
            ct = np.array([float.fromhex(x) for x in rec[("ctab", l)][1:]]).reshape(n, 5)
            if n < c:
                assert ("plain", l) in rec and ("chunk", l) not in rec, (npts, l, c)
                continue
            chunked += 1
            rows, stride = (n, (n + 15) // 16 * 16) if mesh else (1, 0)
            assert rec[("chunk", l)] == [str(x) for x in (n, n // c, rows, stride, stride)]
            ref = XC.tables(ct, c)
            for tag in ("g", "v", "w", "SL", "SG", "SQ"):
                got = np.array([float.fromhex(x) for x in rec[(tag, l)]]).reshape(rows, -1)
                want = ref[tag][:rows]
                assert got.shape == want.shape and np.array_equal(got, want), (npts, mesh, c, l, tag)
                assert np.array_equal(np.signbit(got), np.signbit(want)), (npts, mesh, c, l, tag, "signed zeros")
                if not mesh:                                      # one row serves every grid row: the reference's rows are all that row
                    assert all(np.array_equal(ref[tag][i], ref[tag][0]) for i in range(1, n - 1)), (tag, "uniform")
            pad = [float.fromhex(x) for x in rec[("pad", l)]]
            assert len(pad) == 3 * rows * ((n + 15) // 16 * 16 - n) and all(x == 0.0 for x in pad)
        assert (chunked >= 1) == (npts - 2 >= c)                 # (n = 63 with c = 64: no level has a separator)


@pytest.fixture(scope="module")
def results(plain_objs, tmp_path_factory):
    """every case through Solver in one worker process (the loader caches its libraries)"""
    out, objs = plain_objs
    so = os.path.join(out, "libmgsolve_xchunkline_mock.so")
    _link(["-shared", "-Wl,-Bsymbolic", "-o", so], objs)
    npz = str(tmp_path_factory.mktemp("xchunkline") / "res.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "xchunkline_mock_worker.py"), so, npz] + [_key(*k) for k in SOLVES + BOTH + ZERO],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(npz)


def _compare(pc, case, ref, it, rn, u, bnorm):
    """line_reference.compare; the four cases whose contraction leaves no right-hand side with clear margins (see the docstring): all of it
    but the assertion on the reference's margins"""
    if (pc, case[0], case[2]) not in UNCLEAR:
        return LR.compare(ref, it, rn, u, bnorm)
    last, before = LR.margins(ref, LR.RTOL)
    assert last <= 0.94 and before >= 1.06 and before / last < 1.875, (last, before)
    assert it == ref["iters"], (it, ref["iters"])
    rn = np.asarray(rn)
    assert len(rn) == it + 1 and abs(bnorm - ref["bnorm"]) <= 1e-13 * ref["bnorm"]
    assert np.abs(rn - ref["rnorm"]).max() <= 1e-12 * ref["rnorm"][0], np.abs(rn - ref["rnorm"]).max() / ref["rnorm"][0]
    assert np.array_equal(np.asarray(u), ref["u"])


def test_no_right_hand_side_clears_the_margins_where_the_contraction_is_slow(orc):
    """why the UNCLEAR cases exist: on every right-hand side tried the last cycle of the x-line solve on mesh 1 contracts by less than the
    factor 1.5 / 0.8 = 1.875 that line_reference's two margins are apart, so no stop decision there can satisfy both"""
    for pc, npts, mesh in sorted(UNCLEAR):
        for rhs in ("manufactured", "rough:1", "rough:2", "rough:3"):
            ref = XC.reference(orc, (npts, LEVELS[npts], mesh, rhs), pc, 16)
            last, before = LR.margins(ref, LR.RTOL)
            assert 1.0 < before / last < 1.875, (pc, npts, rhs, last, before)


def _calls(pc, xc, yc, case, it):
    """the execution counts of `it` cycles in the worker's order: plain y forward, backward, plain x forward, backward, the four chunked y
    passes, the four chunked x passes.  A smoothing is 3 sweeps, 2 per cycle on every level but the coarsest, 1 there; xline: all x;
    altline: sweeps 0 and 2 in y, sweep 1 in x"""
    npts, levels = case[0], case[1]
    ysw, xsw = (0, 3) if pc == "xline" else (2, 1)
    py = px = cy = cx = 0
    for l in range(levels):
        n = (npts - 1) // (1 << l) - 1
        k = it * (1 if l == levels - 1 else 2)
        if yc >= 2 and n >= yc:
            cy += k * ysw
        else:
            py += k * ysw
        if xc > 0 and n >= xc:
            cx += k * xsw
        else:
            px += k * xsw
    return [py, py, px, px] + [cy] * 4 + [cx] * 4


@pytest.mark.parametrize("pc,xc,yc,case", SOLVES + BOTH, ids=[_key(*k) for k in SOLVES + BOTH])
def test_chunked_solve_over_the_mock_equals_the_reference(orc, results, pc, xc, yc, case):
    """(c)"""
    k = _key(pc, xc, yc, case) + ":"
    ref = XC.reference(orc, case, pc, xc, yc)
    it = int(results[k + "it"])
    _compare(pc, case, ref, it, results[k + "rn"], results[k + "u"], float(results[k + "bnorm"]))
    want = _calls(pc, xc, yc, case, it)
    assert (want[8] > 0) == (case[0] - 2 >= xc) and (yc == 0 or want[4] > 0)      # (npts 33 with c = 32: no level has a separator, the plain sweep everywhere)
    assert list(results[k + "calls"]) == want, (results[k + "calls"], want)
    for tag in ("graph0", "fuse0"):
        assert int(results[k + tag + "_it"]) == it
        assert np.array_equal(results[k + tag + "_rn"], results[k + "rn"]) and np.array_equal(results[k + tag + "_u"], results[k + "u"]), tag


@pytest.mark.parametrize("pc,xc,yc,case", ZERO, ids=[_key(*k) for k in ZERO])
def test_xline_chunk_0_is_the_solver_without_the_keyword(orc, results, pc, xc, yc, case):
    """(e): the default leaves today's code paths and bits: the plain x sweeps of the reference, none of the four passes"""
    k = _key(pc, xc, yc, case) + ":"
    ref = XC.reference(orc, case, pc, 0, yc)
    it = int(results[k + "it"])
    LR.compare(ref, it, results[k + "rn"], results[k + "u"], float(results[k + "bnorm"]))
    want = _calls(pc, 0, yc, case, it)
    assert want[8:] == [0] * 4 and list(results[k + "calls"]) == want, (results[k + "calls"], want)
    for tag in ("nokw", "graph0", "fuse0"):
        assert int(results[k + tag + "_it"]) == it
        assert np.array_equal(results[k + tag + "_rn"], results[k + "rn"]) and np.array_equal(results[k + tag + "_u"], results[k + "u"]), tag


def test_a_link_without_mg_xline_chunk_refuses_by_name():
    """the existing CPU-tier links (tests/mock_mgk_xline.cpp + mg_solver.c + mg_comm.c + mg_line.c + mg_xline.c, and the one of
    tests/test_chunkline_cpu.py with mg_line_chunk.c) know none of the four kernels and need no new symbol; xline_chunk > 0 is refused there
    with the reason, xline_chunk = 0 is served"""
    for tag, mock, extra in (("unlinked", "mock_mgk_xline.cpp", ()), ("unlinked_y", "mock_mgk_chunkline.cpp", ("mg_line_chunk.c",))):
        out, objs = _compile(tag, [], [os.path.join(HERE, mock)] + [os.path.join(CSRC, f) for f in ("mg_solver.c", "mg_comm.c", "mg_line.c", "mg_xline.c") + extra])
        so = os.path.join(out, f"libmgsolve_xchunkline_{tag}.so")
        _link(["-shared", "-Wl,-Bsymbolic", "-o", so], objs)
        p = subprocess.run([sys.executable, os.path.join(HERE, "xchunkline_mock_worker.py"), so, "--unlinked"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:]


@pytest.fixture(scope="module")
def san_exe():
    """the same sources as one executable with -fsanitize=address,undefined, built once"""
    out, objs = _compile("san", SAN, _sources() + [os.path.join(HERE, "san_xchunkline.c")])
    exe = os.path.join(out, "san_xchunkline")
    _link(SAN + ["-o", exe], objs)
    return exe


@pytest.mark.parametrize("pc,xc,yc,case", SAN_CASES, ids=[_key(*k) for k in SAN_CASES])
def test_chunked_solve_under_sanitizers(orc, san_exe, tmp_path, pc, xc, yc, case):
    """(d): under -fsanitize=address,undefined no report (leaks included: mg_solver_destroy frees the tables and the separator workspace, a
    refused creation leaves nothing), the refusals, two solves and a destroy, and results that pass the same bars"""
    npts, levels, mesh, rhs = case
    ref = XC.reference(orc, case, pc, xc, yc)
    rhsfile = "-"
    if rhs != "manufactured":
        import rhs_cases
        rhsfile = str(tmp_path / "rhs.bin")
        rhs_cases.uniform(2, npts, int(rhs.split(":")[1])).tofile(rhsfile)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    txt = str(tmp_path / "out.txt")
    p = subprocess.run([san_exe, str({"xline": 2, "altline": 3}[pc]), str(npts), str(levels), str(mesh), repr(LR.SCALE), str(xc), str(yc), rhsfile, txt],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:]
    got = {ln.split(" ", 1)[0]: ln.split()[1:] for ln in open(txt)}
    for tag in ("solve", "again"):
        rn = np.array(got[tag + "_rnorm"], dtype=float)
        _compare(pc, case, ref, int(got[tag + "_iters"][0]), rn, np.array(got[tag + "_u"], dtype=float), ref["bnorm"])


def test_the_entry_points_are_built_and_only_mg_xline_chunk_names_the_kernels():
    """the four kernels are declared and exported by libmgk.so, the hooks by libmgpetsc.so; of the host sources only mg_xline_chunk.c names
    them; mg_config and MgConfig carry the field directly before line_chunk"""
    hk, hs = open(os.path.join(ROOT, "include", "mgk.h")).read(), open(os.path.join(ROOT, "include", "mgsolve.h")).read()
    assert all(k + "(" in hk for k in KERNELS) and "int xline_chunk;" in hs
    assert hs.index("int pc_type;") < hs.index("int xline_chunk;") < hs.index("int line_chunk;")
    lib = os.path.join(ROOT, "multigrid_petsc_amd")
    Lk = ctypes.CDLL(os.path.join(lib, "libmgk.so"))
    Lp = ctypes.CDLL(os.path.join(lib, "libmgpetsc.so"))
    assert all(hasattr(Lk, k) for k in KERNELS)
    assert hasattr(Lp, "mg_xline_chunk_smooth") and hasattr(Lp, "mg_xline_chunk_tables")
    for f in sorted(os.listdir(CSRC)) + [os.path.join("driver", "mgpoisson.c")]:
        if not f.endswith(".c") or f == "mg_xline_chunk.c":
            continue
        text = open(os.path.join(CSRC, f)).read()
        for name in KERNELS:
            assert name not in text, f"{f} names {name}"
    text = open(os.path.join(CSRC, "mg_xline_chunk.c")).read()
    assert all(k + "(" in text for k in KERNELS)
    from multigrid_petsc_amd.mgk import Mgk  # noqa: F401  (the signatures are declared with the others)
    assert all('"%s"' % k in open(os.path.join(lib, "mgk.py")).read() for k in KERNELS)
    from multigrid_petsc_amd.solver import MgConfig
    names = [f[0] for f in MgConfig._fields_]
    assert names[-2:] == ["xline_chunk", "line_chunk"]
    cfg = MgConfig()
    Lp.mg_config_default(ctypes.byref(cfg))
    assert cfg.xline_chunk == 0 and cfg.line_chunk == 0


def test_own_driver_takes_xline_chunk(tmp_path):
    """mgpoisson -xline_chunk c: a period that is no multiple of 16, or one with point Jacobi, stops with the library's message before any solve"""
    exe = os.path.join(ROOT, "multigrid_petsc_amd", "mgpoisson")
    assert os.path.exists(exe), "mgpoisson is not built (csrc/Makefile builds it with the libraries)"
    assert '"-xline_chunk"' in open(os.path.join(CSRC, "driver", "mgpoisson.c")).read()
    for args, msg in ((["-pc_type", "altline", "-xline_chunk", "8"], "xline_chunk must be"), (["-xline_chunk", "16"], "not jacobi or yline")):
        p = subprocess.run([exe, "-npts", "17", "-levels", "3"] + args, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert p.returncode == 1 and msg in p.stdout, (args, p.returncode, p.stdout)
