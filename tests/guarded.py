"""Guarded(mgk, poison=True): a drop-in for the `mgk` fixture object (multigrid_petsc_amd/mgk.py Mgk) under which a test body's device buffers are
watched for WHERE a call stores, the half of the kernel ABI's contract that a comparison of interiors cannot see (include/mgk.h, Conventions):

    A call writes the interior of its output fields, and within an output's allocation it may store zeros into the ghost ring and row
    padding.  Where they held 0 they hold 0 afterwards.  A call never writes outside the allocation.  The slab and range forms write only
    the planes / rows they are given.

 * guards: every allocation sits between two zones of GUARD_DOUBLES doubles that hold a fixed finite sentinel; the pointer handed out is
   base + 2 KiB (the 128-byte row alignment holds).  from_field*, raw_field, download of a known buffer and free download the whole allocation
   and assert that both zones are bitwise intact.
 * layout: to_field* lays the field out on the host with numpy from the members of the geometry (offset = org + k*plane + i*pitch + j) and
   uploads it; from_field* takes the interior out on the host.  Neither goes through mgk_pack_* / mgk_unpack_*.
 * frame: from_field* asserts that every cell of the allocation outside the interior is 0 (+0 or -0: the full-row kernels store zeros there on
   purpose).  A buffer that came from upload() -- a slab field with halo planes, say -- is held to the contract's own words: the cells that were
   0 when it was uploaded.
 * poison: field(g) / field32(g32) return a field whose ghost ring and padding are 0 and whose interior holds a quiet NaN with a recognisable
   payload, so a call that skips an output cell, or reads its output, leaves a NaN where the body compares.  (mgk_malloc zero-fills, and the
   bodies reuse one output buffer over their tuning variants: without the poison the run before hands such a call the right answer.)
 * a body's own mgk_memset0 over a whole field(g) / field32(g) output -- the bodies clear their outputs straight after allocating them and between
   tuning variants -- would wipe the poison before the kernel under test runs: the proxy lets the zeros land and poisons the interior again.
   An output whose content the body has fetched is poisoned again before the next library call that is handed it, so a body that reuses one
   output over its variants without clearing it gives every call a poisoned one.  The proxy counts, per watched entry point, the calls that
   were handed a still-poisoned output (`poisoned_calls`).
 * scratch: the context's reduction scratch (mgk_debug_partials: 3 x 16384 doubles that every sum of squares, dot product and error norm
   deposits its per-block / per-wave partials in, never cleared, shared by all of them) is filled with the same NaN before every call of an
   entry point of REDUCERS, the whole allocation: a slot that the finishing kernel adds up and the launch did not write turns the returned sum
   into NaN, where without the fill it holds the right value from the tuning variant before, or zero.  The range forms gather the partials
   of several calls before one mgk_partials_finish: only a call with part_off == 0 opens such a group and is preceded by the fill.  The
   proxy counts the calls so treated per entry point (`scratch_poisoned_calls`).
 * L is a recording wrapper: it forwards every attribute and logs the name of each function called (`calls`).

Not asserted: out-of-bounds READS, and what the padding of an input may hold.  Neither is in the contract.

HostMgk(lib) is the same surface over a host stand-in of the ABI (tests/mock_mgk.cpp built as a shared library): the dry run of the CPU tier.
Plain helper module: no fixtures.  Test infrastructure only."""
import ctypes as C
import struct
import types

import numpy as np

from multigrid_petsc_amd.mgk import Geom, Mgk, MgkError, _sigs

GUARD_DOUBLES = 256
GUARD_BYTES = 8 * GUARD_DOUBLES
SENTINEL = struct.unpack("<d", struct.pack("<Q", 0x4B1DF00DCAFE0123))[0]          # finite, about 1.7e54, an unlikely value of any field
POISON64_BITS, POISON32_BITS = 0x7FF80000DEADBEEF, 0x7FC0BEEF                  # quiet NaNs
_GUARD = np.full(GUARD_DOUBLES, SENTINEL).view(np.uint8)


def poison_value(dtype):
    if np.dtype(dtype) == np.float64:
        return np.array([POISON64_BITS], dtype=np.uint64).view(np.float64)[0]
    return np.array([POISON32_BITS], dtype=np.uint32).view(np.float32)[0]


def is_poison(a):
    """elementwise: the cell still holds the poison's bits"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) == POISON64_BITS if a.dtype == np.float64 else a.view(np.uint32) == POISON32_BITS


def interior(g, flat):
    """(nz, ny, nx) strided view of the interior of a flat padded array: offset = org + k*plane + i*pitch + j, written out"""
    it = flat.itemsize
    nz = g.nz if g.dim == 3 else 1
    last = g.org + (nz - 1) * g.plane + (g.ny - 1) * g.pitch + g.nx - 1
    assert 0 <= g.org and last < flat.size, f"geometry reaches offset {last} of an array of {flat.size}"
    return np.lib.stride_tricks.as_strided(flat[g.org:], shape=(nz, g.ny, g.nx), strides=(g.plane * it, g.pitch * it, it))


def layout(g, compact, dtype=np.float64):
    """compact lexicographic (k*ny + i)*nx + j -> flat padded array of g.total elements, ghost ring and padding 0"""
    flat = np.zeros(g.total, dtype=dtype)
    nz = g.nz if g.dim == 3 else 1
    interior(g, flat)[...] = np.asarray(compact, dtype=dtype).reshape(nz, g.ny, g.nx)
    return flat


def kij(g, off):
    """(k, i, j) of a flat offset of geometry g: k = -1 / nz and i = -1 / ny are the ghost planes / rows, j < 0 or j >= nx the row padding"""
    xoff = g.org % g.pitch
    rel = int(off) - (g.org - xoff - g.pitch - (g.plane if g.dim == 3 else 0))          # from the start of ghost row -1 of ghost plane -1
    k = rel // g.plane - 1 if g.dim == 3 else 0
    r = rel % g.plane if g.dim == 3 else rel
    return (k, r // g.pitch - 1, r % g.pitch - xoff)


# the entry points whose launcher hands the context's reduction scratch to a kernel (tests/test_reduction_scratch_cpu.py derives the same set from
# csrc/*.hip); value: the index of the call's part_off argument, None where the call reduces its own partials
REDUCERS = {
    "mgk_residual_sumsq_f64": None, "mgk_jacobi_sumsq_f64": None, "mgk_jacobi_sumsq_store_f64": None, "mgk_jacobi_sumsq_range_f64": 10,
    "mgk_jacobi2_sumsq_f64": None, "mgk_jacobi2_sumsq_mid_f64": None, "mgk_jacobi2_sumsq_slab_f64": 14, "mgk_jacobi2_sumsq_mid_slab_f64": 14,
    "mgk_jacobi2_2d_sumsq_f64": None, "mgk_jacobi2_2d_sumsq_rowcoef_f64": None, "mgk_sumsq_f64": None, "mgk_error_sums_f64": None,
    "mgk_flat_dot": None, "mgk_residual_f64_to_f32": None, "mgk_residual_f64_to_f32_jz": None, "mgk_correct_residual_f64_f32": None,
    "mgk_correct_residual_f64_f32_jz": None, "mgk_jacobi_sumsq_rowcoef_f64": None, "mgk_residual_sumsq_rowcoef_f64": None,
    "mgk_jacobi3_2d_sumsq_f64": None, "mgk_jacobi3_2d_sumsq_store_f64": None, "mgk_cheby3_2d_sumsq_f64": None, "mgk_jacobi3_sumsq_f64": None,
    "mgk_jacobi3_sumsq_mid_f64": None, "mgk_multi_dot_f64": None, "mgk_multi_axpy_sumsq_f64": None,
}


class _Buf:
    def __init__(self, base, nbytes, geom=None, dtype=None, init=None, output=False):
        self.base, self.nbytes, self.geom, self.dtype, self.init = base, nbytes, geom, dtype, init
        self.output = output                # handed out by field() / field32(): an output of the body
        self.poisoned = False               # its interior holds the poison and nothing the proxy knows of has written it since
        self.taken = False                  # the body has fetched its content: before the next call that is handed it, it is poisoned again


class _Fn:
    """one function of the library: logs its name, forwards the call and the ctypes attributes (restype / argtypes)"""

    def __init__(self, name, fn, log, owner):
        self.__dict__.update(_name=name, _fn=fn, _log=log, _owner=owner)

    def __call__(self, *a):
        self._log.append(self._name)
        if self._owner is not None:
            self._owner._before(self._name, a)
        rc = self._fn(*a)
        if self._owner is not None:
            self._owner._after(self._name, a, rc)
        return rc

    def __getattr__(self, k):
        return getattr(self._fn, k)

    def __setattr__(self, k, v):
        setattr(self._fn, k, v)


class RecordingLib:
    def __init__(self, lib, owner=None):
        self.__dict__.update(_lib=lib, calls=[], _fns={}, _owner=owner)

    def __getattr__(self, name):
        if name.startswith("_"):
            return getattr(self._lib, name)
        if name not in self._fns:
            self._fns[name] = _Fn(name, getattr(self._lib, name), self.calls, self._owner)
        return self._fns[name]


class Guarded:
    def __init__(self, mgk, poison=True):
        self.inner, self.poison = mgk, poison
        self.L = RecordingLib(mgk.L, self)
        self.watch = frozenset()            # entry points whose calls are looked at: did one get a still-poisoned field?
        self.poisoned_calls = {}            # name -> calls of it that were handed at least one still-poisoned output field
        self.repoisoned = 0                 # whole-field mgk_memset0 calls of the body after which the poison was put back
        self.scratch_poisoned_calls = {}    # name -> calls of a REDUCERS entry before which the whole reduction scratch was filled with the poison
        self._scratch = None                # (device address, doubles) of the context's reduction scratch
        self.ctx, self.symbols = mgk.ctx, mgk.symbols
        self.live = {}                      # handed-out address -> _Buf
        self.frame_checks = self.guard_checks = self.whole_downloads = 0    # whole_downloads: allocations handed back to the body in full

    # what the bodies take from Mgk unchanged: these use self.L and self.ctx alone, so the calls they make are logged
    _chk, geom, geom32, tail_cycle_line = Mgk._chk, Mgk.geom, Mgk.geom32, Mgk.tail_cycle_line
    coef = staticmethod(Mgk.coef)

    @property
    def calls(self):
        return self.L.calls

    def sync(self):
        self.inner.sync()

    def last_error(self):
        """the message of the calling thread's last refused call"""
        return self.L.mgk_last_error().decode()

    # -- what the body does through L --
    _WRITERS = {"mgk_memset0": 1, "mgk_h2d": 1, "mgk_h2d_async": 1, "mgk_d2d": 1}          # name -> index of the destination pointer

    def _known(self, a):
        if isinstance(a, C.c_void_p):
            a = a.value
        return self.live.get(a) if isinstance(a, int) else None

    def _poison_again(self, buf):
        flat = np.zeros(buf.geom.total, dtype=buf.dtype)
        interior(buf.geom, flat)[...] = poison_value(buf.dtype)
        self.inner.sync()
        self._h2d(buf.base.value + GUARD_BYTES, flat)
        buf.poisoned, buf.taken = True, False
        self.repoisoned += 1

    # -- the reduction scratch --
    def scratch(self):
        """(device address, doubles allocated) of the context's reduction scratch"""
        if self._scratch is None:
            n = C.c_long()
            p = self.inner.L.mgk_debug_partials(self.ctx, C.byref(n))
            assert p and n.value > 0, "mgk_debug_partials"
            self._scratch = (p if isinstance(p, int) else p.value, n.value)
        return self._scratch

    def poison_scratch(self):
        addr, n = self.scratch()
        self.inner.sync()
        self._h2d(addr, np.full(n, poison_value(np.float64)))

    def read_scratch(self):
        addr, n = self.scratch()
        self.inner.sync()
        return self.inner.download(C.c_void_p(addr), n)

    def _before(self, name, args):
        if name in REDUCERS and self.poison:
            off = REDUCERS[name]
            off = 0 if off is None else (args[off].value if hasattr(args[off], "value") else int(args[off]))
            if off == 0:                                # (a later range of a group must find the partials of the ranges before it)
                self.poison_scratch()
                self.scratch_poisoned_calls[name] = self.scratch_poisoned_calls.get(name, 0) + 1
        if name not in self._WRITERS and self.poison:
            for b in map(self._known, args):            # an output whose result the body has taken already: the next kernel must not find it there
                if b is not None and b.output and b.taken:
                    self._poison_again(b)
        if name in self.watch and any(b is not None and b.poisoned for b in map(self._known, args)):
            self.poisoned_calls[name] = self.poisoned_calls.get(name, 0) + 1

    def _after(self, name, args, rc):
        """a body's mgk_memset0 over a whole output field would wipe the poison before the kernel under test runs (the bodies clear their
        outputs between tuning variants, and straight after allocating them): the zeros land, then the interior is poisoned again.  Any other
        write of the body into a known buffer ends its poisoned state"""
        if name not in self._WRITERS or len(args) <= 2:
            for b in map(self._known, args):            # a kernel that was handed the field may have written it
                if b is not None:
                    b.poisoned = False
            return
        buf = self._known(args[self._WRITERS[name]])
        if buf is None:
            return
        n = args[2].value if hasattr(args[2], "value") else int(args[2])
        if name == "mgk_memset0" and rc == 0 and self.poison and buf.output and n == buf.nbytes:
            self._poison_again(buf)
        else:
            buf.poisoned = buf.taken = False

    # -- allocations between guards --
    @staticmethod
    def _addr(p):
        return p.value if isinstance(p, C.c_void_p) else int(p)

    def _h2d(self, addr, arr):
        self.inner._chk(self.inner.L.mgk_h2d(self.ctx, C.c_void_p(addr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def _new(self, nbytes, content=None, **kw):
        base = self.inner.alloc(2 * GUARD_BYTES + nbytes)
        if content is None:                 # zero-filled by mgk_malloc
            self._h2d(base.value, _GUARD)
            self._h2d(base.value + GUARD_BYTES + nbytes, _GUARD)
        else:
            img = np.concatenate([_GUARD, np.ascontiguousarray(content).reshape(-1).view(np.uint8), _GUARD])
            assert img.nbytes == 2 * GUARD_BYTES + nbytes
            self._h2d(base.value, img)
        p = C.c_void_p(base.value + GUARD_BYTES)
        self.live[p.value] = _Buf(base, nbytes, **kw)
        return p

    def _fetch(self, p, what):
        """the bytes of a known allocation, after the check of its two guard zones"""
        buf = self.live[self._addr(p)]
        img = np.empty(2 * GUARD_BYTES + buf.nbytes, dtype=np.uint8)
        self.inner.sync()
        self.inner._chk(self.inner.L.mgk_d2h(self.ctx, img.ctypes.data_as(C.c_void_p), buf.base, img.nbytes))
        self.guard_checks += 1
        buf.poisoned, buf.taken = False, buf.output          # the body looks at it: a kernel has written it by now
        for zone, lo in (("before", 0), ("after", GUARD_BYTES + buf.nbytes)):
            bad = np.flatnonzero(img[lo:lo + GUARD_BYTES] != _GUARD)
            if bad.size:
                at = int(bad[0]) - GUARD_BYTES if zone == "before" else buf.nbytes + int(bad[0])
                where = ""
                if buf.geom is not None:
                    it = np.dtype(buf.dtype).itemsize
                    where = f", element {at // it} = (k, i, j) {kij(buf.geom, at // it)} of its geometry"
                raise AssertionError(f"{what}: guard zone {zone} the allocation of {buf.nbytes} bytes was written: {bad.size} bytes, the first at "
                                     f"byte {at} of the allocation{where}")
        return buf, img[GUARD_BYTES:GUARD_BYTES + buf.nbytes]

    def alloc(self, nbytes):
        return self._new(int(nbytes))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        return self._new(arr.nbytes, arr, init=arr.reshape(-1).copy())

    def download(self, p, n):
        if self._addr(p) not in self.live:
            return self.inner.download(p, n)
        buf, raw = self._fetch(p, "download")
        assert 8 * n <= buf.nbytes, f"download of {n} doubles from an allocation of {buf.nbytes} bytes"
        self.whole_downloads += 8 * n + 8 > buf.nbytes
        return raw[:8 * n].view(np.float64).copy()

    def free(self, p):
        buf, _ = self._fetch(p, "free")
        del self.live[self._addr(p)]
        self.inner.free(buf.base)

    def assert_no_leaks(self):
        assert not self.live, f"{len(self.live)} buffers were not freed"

    def release(self):
        """free what a failed body left behind (no checks)"""
        for buf in self.live.values():
            self.inner.free(buf.base)
        self.live.clear()

    # -- fields --
    def _field(self, g, dtype):
        flat = np.zeros(g.total, dtype=dtype)
        if self.poison:
            interior(g, flat)[...] = poison_value(dtype)
        gg = Geom.from_buffer_copy(g)
        if not self.poison:
            return self._new(flat.nbytes, geom=gg, dtype=dtype, output=True)
        p = self._new(flat.nbytes, flat, geom=gg, dtype=dtype, output=True)
        self.live[p.value].poisoned = True
        return p

    def field(self, g):
        return self._field(g, np.float64)

    def field32(self, g32):
        return self._field(g32, np.float32)

    def _to(self, g, compact, dtype):
        flat = layout(g, np.asarray(compact, dtype=np.float64).ravel(), dtype)
        return self._new(flat.nbytes, flat, geom=Geom.from_buffer_copy(g), dtype=dtype)

    def to_field(self, g, compact):
        return self._to(g, compact, np.float64)

    def to_field32(self, g32, compact):
        return self._to(g32, compact, np.float32)

    def _from(self, g, f, dtype, what):
        buf, raw = self._fetch(f, what)
        it = np.dtype(dtype).itemsize
        assert g.total * it <= buf.nbytes, f"{what}: geometry of {g.total} elements on an allocation of {buf.nbytes} bytes"
        flat = raw[:g.total * it].view(dtype)
        out = np.ascontiguousarray(interior(g, flat)).ravel()
        frame = flat.copy()
        interior(g, frame)[...] = 0
        if buf.geom is None and buf.init is not None and buf.init.nbytes >= frame.nbytes:
            was = buf.init.view(np.uint8)[:frame.nbytes].view(dtype)       # an uploaded buffer: the cells that held 0 hold 0
            frame[was != 0] = 0
        self.frame_checks += 1
        bad = np.flatnonzero(frame != 0)                                      # NaN != 0; -0.0 == 0
        if bad.size:
            first = [(kij(g, o), float(frame[o])) for o in bad[:8]]
            raise AssertionError(f"{what}: frame not zero: {bad.size} cells of the ghost ring / row padding of a {g.nx} x {g.ny} x {g.nz} field "
                                 f"hold a non-zero, the first ((k, i, j), value): {first}")
        return out

    def from_field(self, g, f):
        return self._from(g, f, np.float64, "from_field")

    def from_field32(self, g32, f):
        return self._from(g32, f, np.float32, "from_field32")

    def raw_field(self, g, f):
        buf, raw = self._fetch(f, "raw_field")
        self.whole_downloads += 8 * g.total + 8 > buf.nbytes
        return raw[:8 * g.total].view(np.float64).copy()


class MissingStandIn(Exception):
    """the host stand-in library does not export this entry point"""


class _HostLib:
    def __init__(self, lib):
        self.__dict__["_lib"] = lib

    def __getattr__(self, name):
        try:
            return getattr(self._lib, name)
        except AttributeError:
            if name.startswith("mgk_"):
                raise MissingStandIn(name) from None
            raise


class HostMgk:
    """the surface of Mgk over a host stand-in library of the kernel ABI; `missing`: the entry points of Mgk's table that it does not export"""

    def __init__(self, path):
        self.L = _HostLib(C.CDLL(path))
        table = _sigs(_Anything())
        self.symbols, self.missing = {}, []
        for name, (res, args) in table.items():
            try:
                f = getattr(self.L, name)
            except MissingStandIn:
                self.missing.append(name)
                continue
            f.restype, f.argtypes = res, args
            self.symbols[name] = (res, args)
        self.ctx = C.c_void_p()
        self._chk(self.L.mgk_ctx_create(C.byref(self.ctx), 0))

    _chk, geom, geom32, alloc, free, sync, field, field32 = Mgk._chk, Mgk.geom, Mgk.geom32, Mgk.alloc, Mgk.free, Mgk.sync, Mgk.field, Mgk.field32
    upload, download, close = Mgk.upload, Mgk.download, Mgk.close
    coef = staticmethod(Mgk.coef)


class _Anything:
    """stands for a library while Mgk's signature table is read: every attribute is an object that takes restype / argtypes"""

    def __getattr__(self, name):
        return types.SimpleNamespace()


# entry points of include/mgk.h with a writable device-field parameter that no case of tests/test_guarded_gpu.py is there for, with the reason
# (kept here, not in a test module: tests/test_kernel_abi_coverage.py takes a name in tests/test_*.py for a test of it)
_LINE = "its own sentinel test: tests/test_line_kernels_gpu.py fills the outputs with a sentinel and compares the raw allocation"
_XLINE = "its own sentinel test: tests/test_xline_kernels_gpu.py fills the outputs with a sentinel and compares the raw allocation"
_CHUNK = "its own sentinel test: tests/test_chunkline_kernels_gpu.py fills the outputs with a sentinel and compares the raw allocation"
_XCHUNK = "its own sentinel test: tests/test_xchunkline_kernels_gpu.py fills the outputs with a sentinel and compares the raw allocation"
_RBGS = "its own sentinel test: tests/test_rbgs_kernels_gpu.py poisons the outputs and compares the raw allocation"
EXEMPT = {
    "mgk_timer_elapsed_ms": "a timer: `ms` is a host double, not a device field",
    "mgk_defer_result": "registers the device slot of the deferred reductions; it stores nothing itself, not a field writer",
    "mgk_stream_triad_f64": "bandwidth probe of the benchmark on flat arrays; no result of the solver depends on it",
    "mgk_peer_allreduce": "a flag kernel of the peer transport (IPC memory of several processes), out of this module's scope",
    "mgk_line_forward_f64": _LINE, "mgk_line_backward_f64": _LINE,
    "mgk_xline_forward_f64": _XLINE, "mgk_xline_backward_f64": _XLINE,
    "mgk_tail_cycle_line_f64": "its own sentinel test: tests/test_line_tail_kernel_gpu.py checks the ghost ring and padding of the raw allocation",
    "mgk_line_chunk_forward_f64": _CHUNK, "mgk_line_chunk_backward_f64": _CHUNK, "mgk_line_chunk_reduce_f64": _CHUNK, "mgk_line_chunk_correct_f64": _CHUNK,
    "mgk_xline_chunk_forward_f64": _XCHUNK, "mgk_xline_chunk_backward_f64": _XCHUNK, "mgk_xline_chunk_reduce_f64": _XCHUNK,
    "mgk_xline_chunk_correct_f64": _XCHUNK,
    "mgk_rbgs_2d_f64": _RBGS, "mgk_prolong_rbgs_2d_f64": _RBGS,
}

__all__ = ["EXEMPT", "REDUCERS", "Guarded", "HostMgk", "MissingStandIn", "MgkError", "SENTINEL", "GUARD_DOUBLES", "interior", "layout", "kij", "is_poison", "poison_value"]
