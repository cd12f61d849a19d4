"""CPU tier of tests/test_reduction_scratch_gpu.py (the context's reduction scratch, mgk_ctx::partials).

1. The completeness gate.  guarded.REDUCERS -- the entry points before which the proxy poisons the scratch, and the key set of the GPU module's
   case, verdict and deferral tables -- must be the set the sources give: a scan of csrc/*.hip finds every function that names the scratch
   (c->partials / a.partials).  An extern "C" entry point that names it is a reducer.  A host helper that names it is a LAUNCHER: the norm is an
   option of it (a template flag or a non-null norm_parts), which a scan of names cannot follow, so LAUNCHERS lists per launcher the entry points
   that take the option and those that reach the launcher without it; every entry point that reaches a launcher must be in one of the two lists.
   A reducing entry point added later fails here until it has a row in REDUCERS, a case, a verdict and a deferral row.
2. The dry run: the bodies of the GPU module over the host stand-ins (tests/mock_mgk*.cpp) where they have the entry point.  The stand-ins
   reduce on the host and leave the scratch alone (the range forms deposit one partial per call), so the run pins the bodies' references, the
   proxy's poisoning, the range groups and the deferral protocol, not the launchers' slot arithmetic."""
import glob
import os
import re

import numpy as np
import pytest

import test_guarded_cpu as GC
import test_guarded_gpu as GG
import test_reduction_scratch_gpu as RS
from guarded import REDUCERS, Guarded, HostMgk, MissingStandIn, is_poison
from oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multigrid_petsc_amd", "csrc")

# functions that name the scratch and hand it to no kernel that writes it
NOT_LAUNCHERS = {
    "ctx_build": "allocates it", "ctx_release": "frees it", "mgk_debug_partials": "hands its address to a test",
    "finish_to_host": "launches the finishing kernels, which read it: every reducer ends here or in a finish of its own",
}
# launcher -> (entry points that take its norm option, entry points that reach it without)
LAUNCHERS = {
    "jacobi2": ("mgk_jacobi2_sumsq_f64 mgk_jacobi2_sumsq_mid_f64 mgk_jacobi2_sumsq_slab_f64 mgk_jacobi2_sumsq_mid_slab_f64",
                "mgk_jacobi2_f64 mgk_jacobi2_f32 mgk_jacobi2_zero_f64 mgk_jacobi2_zero_f32 mgk_jacobi2_slab_f64 mgk_jacobi2_slab_f32"),
    "jacobi2_2d": ("mgk_jacobi2_2d_sumsq_f64 mgk_jacobi2_2d_sumsq_rowcoef_f64", "mgk_jacobi2_2d_f64 mgk_jacobi2_2d_rowcoef_f64"),
    "bridge_residual": ("mgk_residual_f64_to_f32 mgk_residual_f64_to_f32_jz mgk_correct_residual_f64_f32 mgk_correct_residual_f64_f32_jz", ""),
    "jacobi3_2d": ("mgk_jacobi3_2d_sumsq_f64 mgk_jacobi3_2d_sumsq_store_f64 mgk_cheby3_2d_sumsq_f64",
                   "mgk_jacobi3_2d_f64 mgk_jacobi3_2d_zero_f64 mgk_prolong_jacobi3_2d_f64 mgk_cheby3_2d_f64 mgk_cheby3_2d_zero_f64 mgk_prolong_cheby3_2d_f64 "
                   "mgk_interp_jacobi3_2d_f64"),
    "jacobi3_3d_launch": ("mgk_jacobi3_sumsq_f64", "mgk_jacobi3_f64"),
    "jacobi3s": ("mgk_jacobi3_sumsq_f64 mgk_jacobi3_sumsq_mid_f64", "mgk_jacobi3_f64 mgk_prolong_jacobi3_f64"),
}
NAMES_SCRATCH = re.compile(r"\bc->partials\b|\ba\.partials\b")
_KEYWORDS = {"if", "for", "while", "switch", "return", "sizeof", "catch", "do", "else", "defined", "static_assert", "decltype", "alignas"}


def _clean(src):
    """comments out, string literals emptied"""
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return re.sub(r'"(?:\\.|[^"\\\n])*"', '""', src)


def _match(src, i, open_, close):
    depth = 0
    for j in range(i, len(src)):
        if src[j] == open_:
            depth += 1
        elif src[j] == close:
            depth -= 1
            if depth == 0:
                return j
    raise AssertionError(f"unbalanced {open_} at {i}")


def functions(src):
    """{name: body} of the function definitions of a cleaned source: name ( parameters ) { body } outside every other function's body"""
    out, pos = {}, 0
    for m in iter(lambda: re.compile(r"\b([A-Za-z_]\w*)\s*\(").search(src, pos), None):
        name, lp = m.group(1), m.end() - 1
        rp = _match(src, lp, "(", ")")
        k = rp + 1
        while k < len(src) and src[k] in " \t\n":
            k += 1
        if name in _KEYWORDS or k >= len(src) or src[k] != "{":
            pos = m.end()
            continue
        end = _match(src, k, "{", "}")
        out[name] = out.get(name, "") + src[k:end + 1]
        pos = end + 1
    return out


def scan():
    """(bodies of every function of csrc/*.hip, the names declared by include/mgk*.h)"""
    bodies = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as fh:
            for name, body in functions(_clean(fh.read())).items():
                bodies[name] = bodies.get(name, "") + body
    return bodies, set(re.findall(r"\b(mgk_\w+)\s*\(", headers()))


def headers():
    """include/mgk.h and the headers of the kernel families beside it (include/mgk_*.h), cleaned"""
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "mgk*.h"))):
        with open(path) as fh:
            out.append(_clean(fh.read()))
    return "\n".join(out)


def reaches(bodies, target):
    """the functions whose body names `target`, or a function that does, and so on"""
    idents = {n: set(re.findall(r"[A-Za-z_]\w*", b)) for n, b in bodies.items()}
    hit, grew = {target}, True
    while grew:
        grew = False
        for n, ids in idents.items():
            if n not in hit and ids & hit:
                hit.add(n)
                grew = True
    return hit - {target}


def test_the_scan_reads_function_bodies():
    src = _clean('static int f(int a) { if (a) { g(a); } return fail(1, "x (y { z"); }\n'
                 'template <int N> __global__ void __launch_bounds__(64 * N) k_x(const A a) { a.partials[0] = 0.0; }\n'
                 '#define CALL(K) hipLaunchKernelGGL(k_x<K>, 1, 1, 0, s, a)\n'
                 'extern "C" int mgk_y(mgk_ctx *c) { A a; a.partials = c->partials; CALL(2); return f(1); } // tail { \n')
    fs = functions(src)
    assert set(fs) == {"f", "k_x", "mgk_y"} and "g(a)" in fs["f"] and NAMES_SCRATCH.search(fs["mgk_y"]) and NAMES_SCRATCH.search(fs["k_x"])
    assert reaches(fs, "f") == {"mgk_y"} and reaches(fs, "k_x") == set()      # (CALL is no function: the kernel is named where the macro is defined)
    bodies, declared = scan()
    assert len(bodies) >= 300 and len(declared) >= 150
    for n in ("k_stencil", "launch_st", "mgk_jacobi_f64", "jacobi3s", "k_multi_dot", "finish_to_host", "mgk_tail_cycle_f64", "mgk_rbgs_2d_f64"):
        assert n in bodies, n
    assert declared <= set(bodies), sorted(declared - set(bodies))[:5]


def test_reducers_are_the_entry_points_that_hand_the_scratch_to_a_kernel():
    bodies, declared = scan()
    named = {n for n, b in bodies.items() if NAMES_SCRATCH.search(b)}
    kernels = {n for n in named if n.startswith("k_")}
    assert kernels and all(re.search(r"\bpartials\s*\[", bodies[k]) for k in kernels)
    stale = sorted(set(NOT_LAUNCHERS) - named)
    assert not stale, f"listed as naming the scratch, but they do not: {stale}"
    host = named - kernels - set(NOT_LAUNCHERS)
    direct = host & declared
    launchers = host - declared
    assert launchers == set(LAUNCHERS), f"host helpers that name the scratch vs the table: {sorted(launchers ^ set(LAUNCHERS))}"
    via = set()
    for launcher, (with_norm, without) in LAUNCHERS.items():
        with_norm, without = set(with_norm.split()), set(without.split())
        reach = reaches(bodies, launcher) & declared
        assert reach == with_norm | without and not with_norm & without, \
            f"{launcher}: entry points that reach it and are in neither list, or listed and do not reach it: {sorted(reach ^ (with_norm | without))}"
        via |= with_norm
    assert direct | via == set(REDUCERS), f"reducing entry points of the sources vs guarded.REDUCERS: {sorted((direct | via) ^ set(REDUCERS))}"
    # the entry points that only read the scratch stay out: the proxy must not wipe the partials they are about to add up
    assert "mgk_partials_finish" not in REDUCERS and "mgk_partials_finish" in reaches(bodies, "finish_to_host")
    # part_off: the index of the argument in the ctypes table and in the header
    h = headers()
    for name, off in REDUCERS.items():
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, h, re.S).group(1).split(",")
        names = [p.split()[-1].lstrip("*") for p in params]
        assert ("part_off" in names) == (off is not None) and (off is None or names[off] == "part_off"), (name, names)


def test_every_reducer_has_a_case_a_verdict_and_a_deferral_row():
    assert set(RS.BUILDERS) == set(REDUCERS) == set(RS.SHAPES)
    assert set(RS.OWN_PROTOCOL) <= set(REDUCERS) and all(len(why.split()) >= 5 for why in RS.OWN_PROTOCOL.values())
    assert set(RS.RANGE_FORMS) == {n for n, off in REDUCERS.items() if off is not None}
    assert {c.values[0] for c in RS.DEFER_CASES} == set(REDUCERS)
    assert set(RS.VERDICT.values()) == {"refits", "refuses"}
    # every case names a launcher with a verdict (the builders run on the host stand-ins' geometry: no kernel is called)
    host = HostMgk(GC._build("mock_mgk_fmg.cpp", "libmock_mgk_scratch.so"))
    orc = Oracle()
    try:
        for name, shapes in RS.SHAPES.items():
            for shape, variants, cap_tuning in shapes:
                assert (-1, -1) in variants and shape[1] % 2 == 1
                G = Guarded(host)
                try:
                    P = RS.Box(G, *shape, "level")
                    P.orc = orc
                    op = RS.BUILDERS[name](P)
                    assert op.name == name and op.launcher in RS.VERDICT, (name, op.launcher)
                    assert (RS.VERDICT[op.launcher] == "refits") == (op.min_cap is not None), name
                    assert op.deferrable == (name not in RS.OWN_PROTOCOL), name
                finally:
                    G.release()
    finally:
        host.close()


# ---- 2. the dry run -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def host():
    m = HostMgk(GC._build("mock_mgk_fmg.cpp", "libmock_mgk_scratch.so"))        # (tests/mock_mgk.cpp and the Krylov stand-ins)
    yield m
    m.close()


def _dry(lib, name, body, *args, **kw):
    if name not in lib.symbols:
        pytest.skip(f"the stand-in library lacks {name}")
    try:
        return body(lib, *args, **kw)
    except MissingStandIn as e:
        pytest.skip(f"the stand-in library lacks {e}")


def _first(params):
    """one shape per entry point: the stand-ins have no dispatch forms"""
    seen, out = set(), []
    for p in params:
        if p.values[0] not in seen:
            seen.add(p.values[0])
            out.append(p)
    return out


@pytest.mark.parametrize("name,shape,variants,cap_tuning,kind", _first(RS._cases()))
def test_default_cap_body_over_the_host_stand_ins(host, orc, name, shape, variants, cap_tuning, kind):
    _dry(host, name, RS.body_default_cap, orc, name, shape, variants[:2], kind, host=True)


@pytest.mark.parametrize("name,shape", _first(RS.RANGE_CASES))
def test_range_group_body_over_the_host_stand_ins(host, orc, name, shape):
    _dry(host, name, RS.body_range_groups, orc, name, shape, "level", host=True)


@pytest.mark.parametrize("name,shape", RS.DEFER_CASES)
def test_deferral_body_over_the_host_stand_ins(host, orc, name, shape):
    _dry(host, name, RS.body_deferred, orc, name, shape)


def test_the_proxy_poisons_the_whole_scratch_before_a_reducer_and_not_inside_a_range_group(host, orc):
    G = Guarded(host)
    P = RS.Box(G, *RS.CUBE, "level")
    P.orc = orc
    try:
        addr, n = G.scratch()
        assert n == 3 * RS.SLOTS
        op = RS.BUILDERS["mgk_sumsq_f64"](P)             # (its stand-in sums on the host: what the scratch holds afterwards is the proxy's fill)
        assert op.call() == 0 and G.scratch_poisoned_calls == {"mgk_sumsq_f64": 1}
        assert np.all(is_poison(G.read_scratch())) and np.all(np.isnan(G.read_scratch()))
        o, np_ = P.out(), RS.C.c_int()
        one = RS._range_call(P, "mgk_jacobi_sumsq_range_f64", o)
        assert one(1, 30, 0, np_) == 0 and one(0, 1, np_.value, np_) == 0
        assert G.scratch_poisoned_calls["mgk_jacobi_sumsq_range_f64"] == 1
        s = G.read_scratch()
        assert not is_poison(s[:2]).any() and np.all(is_poison(s[2:]))           # (the stand-in deposits one partial per call)
        Q = Guarded(host, poison=False)
        Q.L.mgk_sumsq_f64(Q.ctx, P.gp, P.db, RS.C.byref(RS.C.c_double()), None)
        assert Q.scratch_poisoned_calls == {}
    finally:
        G.release()


def test_the_stand_in_cap_setter_follows_the_header(host):
    L = host.L
    n = RS.C.c_long()
    assert L.mgk_debug_partials(host.ctx, RS.C.byref(n)) and n.value == 3 * RS.SLOTS
    for bad in (-1, RS.SLOTS + 1):
        assert L.mgk_debug_set_max_partials(host.ctx, bad) == RS.EINVAL
    for ok in (1, RS.SLOTS, 0):
        assert L.mgk_debug_set_max_partials(host.ctx, ok) == 0
