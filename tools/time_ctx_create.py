#!/usr/bin/env python3
"""Time mgk_ctx_create in a fresh process: what a program pays once before its first solve.  One line of JSON, milliseconds.

    python tools/time_ctx_create.py [--lib path/to/libmgk.so]

init_ms     mgk_device_count: the HIP runtime comes up (not part of the create)
create_ms   the first mgk_ctx_create: streams, scratch, events, and the code object of EVERY translation unit of the library loaded
            (MGK_PRELOAD_UNIT, csrc/mgk_dev.hpp) -- about 2 ms per unit was the estimate, this measures it
again_ms    a second create in the same process: the same without the loads
Run it several times, one process at a time; compare two builds by alternating them."""
import argparse
import ctypes
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multigrid_petsc_amd", "libmgk.so"))
    args = ap.parse_args()
    L = ctypes.CDLL(os.path.abspath(args.lib))
    L.mgk_last_error.restype = ctypes.c_char_p
    t0 = time.perf_counter()
    n = L.mgk_device_count()
    t1 = time.perf_counter()
    if n < 1:
        sys.exit("no HIP device visible")
    out = {"lib": os.path.relpath(args.lib), "init_ms": round((t1 - t0) * 1e3, 3)}
    ctxs = []
    for key in ("create_ms", "again_ms"):
        c = ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = L.mgk_ctx_create(ctypes.byref(c), 0)
        t1 = time.perf_counter()
        if rc:
            sys.exit("mgk_ctx_create: " + L.mgk_last_error().decode())
        out[key] = round((t1 - t0) * 1e3, 3)
        ctxs.append(c)
    L.mgk_ctx_destroy.argtypes = [ctypes.c_void_p]
    for c in ctxs:
        L.mgk_ctx_destroy(c)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
