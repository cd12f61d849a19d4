"""Aids of tests/test_cg_kernels_gpu.py that call plumbing entry points of the kernel ABI (stream capture): kept out of the test module, because
tests/test_kernel_abi_coverage.py takes a name in tests/test_*.py for a test of it.  Test infrastructure only."""
import contextlib
import ctypes as C


@contextlib.contextmanager
def capturing(mgk):
    """the compute stream of the context is being captured inside the body; the (empty) recording is thrown away afterwards"""
    L = mgk.L
    L.mgk_capture_begin.restype, L.mgk_capture_begin.argtypes = C.c_int, [C.c_void_p]
    L.mgk_capture_end.restype, L.mgk_capture_end.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]
    L.mgk_graph_destroy.restype, L.mgk_graph_destroy.argtypes = None, [C.c_void_p, C.c_void_p]
    mgk._chk(L.mgk_capture_begin(mgk.ctx))
    try:
        yield
    finally:
        ge = C.c_void_p()
        rc = L.mgk_capture_end(mgk.ctx, C.byref(ge))
        if rc == 0 and ge:
            L.mgk_graph_destroy(mgk.ctx, ge)
