"""CPU tier of the guarded-buffer proxy (tests/guarded.py).

1. The proxy catches what it is for.  tests/mock_mgk_faulty.cpp holds five host functions with the signature of mgk_jacobi_f64, one right and four
   wrong: a non-zero stored into the ghost column j = nx (caught by the frame check), a store one element past g->total (caught by the guard), the
   last interior row skipped, and the old content of unew added into the result (both caught through the poison: the comparison with the oracle
   finds NaN and says "differs").  With poison=False the last two pass -- the skipped row against a buffer that already holds the answer (an output
   reused over tuning variants), the added content against the zero-filled buffer an allocation starts as (where the answer is already there it doubles
   it, which any comparison sees).  That is the blind spot the poison closes.
2. The case list of tests/test_guarded_gpu.py over tests/mock_mgk.cpp built as a shared library: the dry run before the GPU, and the pin of the
   stand-ins' own claim that they touch exactly the extents the HIP kernels touch.  A case whose entry points the stand-ins lack is skipped with
   the missing name.
   Every case that is not listed with a reason must hand each entry point it covers an output that still holds the poison (the proxy undoes the
   bodies' own memsets of their outputs).
3. The completeness gate: every entry point of include/mgk.h with a writable device-field parameter is in some case's covers or in EXEMPT with a
   reason; a stale exemption fails."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_guarded_gpu as GG
from coef_cases import dense_field, distinct_coef, np_sweep
from guarded import GUARD_DOUBLES, SENTINEL, Guarded, HostMgk, MissingStandIn, interior, is_poison, kij, layout
from oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SC = 6.0 / 7.0


def _build(src, name):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "_san")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-ffp-contract=off", "-D_POSIX_C_SOURCE=200809L", "-I" + os.path.join(ROOT, "include"),
                        "-I" + HERE, "-shared", "-Wl,-Bsymbolic", os.path.join(HERE, src), "-o", so, "-lm", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return so


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def faulty():
    m = HostMgk(_build("mock_mgk_faulty.cpp", "libmock_mgk_faulty.so"))
    yield m
    m.close()


@pytest.fixture(scope="module")
def host():
    m = HostMgk(_build("mock_mgk.cpp", "libmock_mgk_guarded.so"))
    yield m
    m.close()


# ---- 0. the proxy's own arithmetic ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,nx,ny,nz", [(2, 1, 1, 1), (2, 5, 121, 1), (3, 7, 3, 2)])
def test_layout_is_the_formula_of_the_header(host, dim, nx, ny, nz):
    g = host.geom(dim, nx, ny, nz)
    compact = 1.0 + np.arange(nx * ny * nz)
    flat = layout(g, compact)
    for k in range(nz):
        for i in range(ny):
            for j in range(nx):
                off = g.org + (k * g.plane if dim == 3 else 0) + i * g.pitch + j
                assert flat[off] == compact[(k * ny + i) * nx + j] and kij(g, off) == (k, i, j)
    assert np.count_nonzero(flat) == compact.size and np.array_equal(interior(g, flat).ravel(), compact)
    assert kij(g, g.org - 1) == (0, 0, -1) and kij(g, g.org + nx) == (0, 0, nx) and kij(g, g.org - g.pitch) == (0, -1, 0)


def test_guards_surround_every_allocation_and_the_poison_is_nan(host):
    G = Guarded(host)
    g = host.geom(3, 7, 5, 3)
    f = G.field(g)
    buf = G.live[f.value]
    assert f.value == buf.base.value + 8 * GUARD_DOUBLES and f.value % 128 == buf.base.value % 128
    whole = host.download(buf.base, 2 * GUARD_DOUBLES + g.total)
    assert np.all(whole[:GUARD_DOUBLES] == SENTINEL) and np.all(whole[-GUARD_DOUBLES:] == SENTINEL) and np.isfinite(SENTINEL)
    body = whole[GUARD_DOUBLES:-GUARD_DOUBLES]
    assert np.all(is_poison(interior(g, body))) and np.all(np.isnan(interior(g, body)))
    assert np.count_nonzero(body) == 7 * 5 * 3                                      # ghost ring and padding are 0
    got = G.from_field(g, f)
    assert np.all(is_poison(got)) and G.frame_checks == 1
    f32 = G.field32(G.geom32(7))
    assert np.all(is_poison(G.from_field32(G.geom32(7), f32)))
    G.free(f)
    G.free(f32)
    G.assert_no_leaks()
    assert "mgk_geom_init_f32" in G.calls and "mgk_pack_f64" not in G.calls and "mgk_unpack_f64" not in G.calls


# ---- 1. deliberately wrong stand-ins ----------------------------------------------------------------------------------------------
def _sweep_case(orc, dim, shape):
    rng = np.random.default_rng(81000 + dim)
    As = distinct_coef(rng, dim)
    u, b = dense_field(rng, *shape), dense_field(rng, *shape)
    return As, u, b, np_sweep(As, SC, b, u).ravel()


def _run(G, fn, g, As, u, b, want, out=None):
    """what a test body does: upload, one call into `out` (a fresh field unless given), compare with the reference, free"""
    du, db = G.to_field(g, u), G.to_field(g, b)
    o = G.field(g) if out is None else out
    fn = getattr(G.L, fn) if isinstance(fn, str) else fn          # through the proxy's library, as a body calls
    try:
        G._chk(fn(G.ctx, C.byref(g), G.coef(As), 1.0 / As[As.size // 2], SC, db, du, o, None))
        got = G.from_field(g, o)
        assert np.array_equal(got, want), f"the sweep differs: {np.count_nonzero(got != want)} of {want.size} cells, {np.count_nonzero(np.isnan(got))} NaN"
        assert np.array_equal(G.from_field(g, du), u.ravel()) and np.array_equal(G.from_field(g, db), b.ravel())
        for p in (du, db) + ((o,) if out is None else ()):
            G.free(p)
    finally:
        if out is None:
            G.release()


def _fn(faulty, name):
    f = getattr(faulty.L, name)
    f.restype, f.argtypes = faulty.symbols["mgk_jacobi_f64"]
    return name


SHAPES = [(2, (5, 9)), (3, (3, 5, 7))]                     # (dim, (nz,) ny, nx)


@pytest.mark.parametrize("dim,shape", SHAPES)
def test_the_proxy_passes_the_right_sweep_and_catches_the_four_wrong_ones(faulty, orc, dim, shape):
    As, u, b, want = _sweep_case(orc, dim, shape)
    g = faulty.geom(dim, shape[-1], shape[-2], shape[0] if dim == 3 else 1)
    G = Guarded(faulty)
    _run(G, _fn(faulty, "faulty_jacobi_right_f64"), g, As, u, b, want)
    _run(G, "mgk_jacobi_f64", g, As, u, b, want)
    G.assert_no_leaks()
    nzl = (shape[0] - 1) if dim == 3 else 0
    for name, word, where in (("faulty_jacobi_ghost_column_f64", "frame not zero", str((nzl, shape[-2] - 1, shape[-1]))),
                              ("faulty_jacobi_past_the_end_f64", "guard zone after", f"byte {8 * g.total} "),
                              ("faulty_jacobi_skips_last_row_f64", "differs", f"{shape[-1]} NaN"),
                              ("faulty_jacobi_adds_old_output_f64", "differs", f"{want.size} NaN")):
        with pytest.raises(AssertionError) as e:
            _run(Guarded(faulty), _fn(faulty, name), g, As, u, b, want)
        assert word in str(e.value) and where in str(e.value), (name, str(e.value))


@pytest.mark.parametrize("dim,shape", SHAPES)
def test_without_the_poison_a_skipped_row_and_a_read_of_the_output_pass(faulty, orc, dim, shape):
    """the blind spot: the zeros of a fresh allocation and an output that the run before filled hide both"""
    As, u, b, want = _sweep_case(orc, dim, shape)
    g = faulty.geom(dim, shape[-1], shape[-2], shape[0] if dim == 3 else 1)
    G = Guarded(faulty, poison=False)
    out = G.field(g)                                        # zero-filled, as Mgk.field hands it out
    _run(G, _fn(faulty, "faulty_jacobi_adds_old_output_f64"), g, As, u, b, want, out=out)      # 0 + the sweep
    _run(G, _fn(faulty, "faulty_jacobi_skips_last_row_f64"), g, As, u, b, want, out=out)       # the buffer already holds the answer
    G.free(out)
    G.release()
    # ... and with the poison on, the same reused buffer is no help once it is a fresh field
    with pytest.raises(AssertionError, match="differs"):
        _run(Guarded(faulty), _fn(faulty, "faulty_jacobi_skips_last_row_f64"), g, As, u, b, want)


@pytest.mark.parametrize("dim,shape", SHAPES)
def test_the_poison_survives_a_bodys_memset_and_the_reuse_of_an_output(faulty, orc, dim, shape):
    """what the imported bodies do to their outputs: clear them with mgk_memset0 straight after allocating them, and reuse one over several calls.
    The proxy poisons the interior again after the memset and before the call that follows a fetch, so both wrong sweeps are still caught"""
    As, u, b, want = _sweep_case(orc, dim, shape)
    g = faulty.geom(dim, shape[-1], shape[-2], shape[0] if dim == 3 else 1)
    G = Guarded(faulty)
    G.watch = frozenset(["faulty_jacobi_adds_old_output_f64"])
    out = G.field(g)
    G._chk(G.L.mgk_memset0(G.ctx, out, 8 * g.total, None))
    assert G.repoisoned == 1 and np.all(is_poison(interior(g, G.raw_field(g, out))))
    G._chk(G.L.mgk_memset0(G.ctx, out, 8 * g.total, None))
    with pytest.raises(AssertionError, match="differs"):
        _run(G, _fn(faulty, "faulty_jacobi_adds_old_output_f64"), g, As, u, b, want, out=out)
    G.release()
    G = Guarded(faulty)
    out = G.field(g)
    _run(G, _fn(faulty, "faulty_jacobi_right_f64"), g, As, u, b, want, out=out)            # the body takes the answer ...
    with pytest.raises(AssertionError, match="differs"):
        _run(G, _fn(faulty, "faulty_jacobi_skips_last_row_f64"), g, As, u, b, want, out=out)   # ... which the next call no longer finds there
    G.release()
    # a memset of part of the field, or of a field that came from to_field, is the body's own business
    G = Guarded(faulty)
    out, inp = G.field(g), G.to_field(g, u)
    G._chk(G.L.mgk_memset0(G.ctx, out, 8 * g.total - 8, None))
    G._chk(G.L.mgk_memset0(G.ctx, inp, 8 * g.total, None))
    assert G.repoisoned == 0 and not np.any(G.raw_field(g, out)) and not np.any(G.raw_field(g, inp))
    G.release()


def test_a_guard_hit_before_the_allocation_and_an_uploaded_halo_buffer(faulty):
    G = Guarded(faulty)
    g = faulty.geom(2, 7, 3, 1)
    f = G.field(g)
    one = np.ones(1)
    faulty._chk(faulty.L.mgk_h2d(faulty.ctx, C.c_void_p(f.value - 8), one.ctypes.data_as(C.c_void_p), 8))
    with pytest.raises(AssertionError, match="guard zone before"):
        G.free(f)
    G.release()
    # an uploaded buffer (a slab field with halo rows): its non-zero frame cells are its own, the cells that were 0 must stay 0
    pad = np.zeros(g.total)
    pad[g.org - g.pitch:g.org - g.pitch + g.nx] = 2.0
    p = G.upload(pad)
    assert np.array_equal(G.from_field(g, p), np.zeros(21))
    faulty._chk(faulty.L.mgk_h2d(faulty.ctx, C.c_void_p(p.value + 8 * (g.org + g.nx)), one.ctypes.data_as(C.c_void_p), 8))
    with pytest.raises(AssertionError, match="frame not zero"):
        G.from_field(g, p)
    G.release()


# ---- 2. the case list over the host stand-ins -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GG.CASES, ids=[GG.case_id(c) for c in GG.CASES])
def test_case_list_over_the_host_stand_ins(host, orc, case):
    body, args, covers = case[:3]
    try:
        GG.run_case(host, orc, body, args, covers, have=set(host.symbols))
    except MissingStandIn as e:                      # an entry point outside `covers` that the body calls on its way
        pytest.skip(f"the stand-in library lacks {e}")


# ---- 3. the completeness gate -----------------------------------------------------------------------------------------------------
def test_header_parse_finds_the_field_writers():
    names = GG.field_writers()
    assert len(names) == len(set(names)) >= 120
    for n in ("mgk_jacobi_f64", "mgk_pack_f32", "mgk_flat_axpy", "mgk_csr_mult_f64", "mgk_tail_cycle_cs_f64", "mgk_sweep_residual_restrict_slab_f64",
              "mgk_scale_to_f64", "mgk_correct_f64_from_f32", "mgk_rbgs_2d_f64"):
        assert n in names
    for n in ("mgk_sumsq_f64", "mgk_residual_sumsq_f64", "mgk_error_sums_f64", "mgk_partials_finish", "mgk_krylov_fetch", "mgk_flat_dot", "mgk_set_tuning"):
        assert n not in names


def test_every_field_writer_has_a_guarded_case_or_an_exemption():
    covered = set().union(*(c[2] for c in GG.CASES))
    gap = set(GG.field_writers()) - covered
    missing = sorted(gap - set(GG.EXEMPT))
    assert not missing, f"entry points that write a device field without a case in tests/test_guarded_gpu.py: {missing}"
    stale = sorted(set(GG.EXEMPT) - gap)
    assert not stale, f"exemptions that a case now covers or the header no longer declares: {stale}"
    for name, why in GG.EXEMPT.items():
        assert len(why.split()) >= 5, name
    assert len(GG.UNPOISONED) <= 3 and all(len(why.split()) >= 5 for why in GG.UNPOISONED.values())
    for table in (GG.IN_PLACE, GG.OWN_FRAMES, GG.OWN_FILL):
        assert all(len(why.split()) >= 2 for why in table.values())
    assert set(GG.IN_PLACE) <= covered and set(GG.OWN_FRAMES) | set(GG.OWN_FILL) <= {c[0] for c in GG.CASES}
    ids = {GG.case_id(c) for c in GG.CASES}
    assert len(ids) == len(GG.CASES) and set(GG.UNPOISONED) <= ids
