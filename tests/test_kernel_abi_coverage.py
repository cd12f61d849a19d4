"""Every entry point of the kernel ABI (include/mgk.h) is named by some test module, or is exempt here with its reason.  A new entry
point without a test fails this, and so does an exemption that a test has made stale: the exemption set must equal the actual gap.
(CPU tier: reads files only.)"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXEMPT = {
    # context, memory, timers, streams, capture and graphs: plumbing every GPU test and the solver go through
    "mgk_set_device": "device selection of a rank; mg_comm.c calls it in the multi-rank tests' workers",
    "mgk_ctx_create": "called by the session fixture (multigrid_petsc_amd/mgk.py Mgk.__init__) under every GPU test",
    "mgk_ctx_destroy": "called by the session fixture's teardown (Mgk.close)",
    "mgk_last_error": "read by Mgk._chk whenever a call fails; tests that expect a refusal see it",
    "mgk_ctx_set_chunk_planes": "a scheduling hint of slab ranks (never changes results); set by mg_solver.c in the multi-rank tests",
    "mgk_malloc": "Mgk.alloc / Mgk.field: every GPU test allocates through it",
    "mgk_free": "Mgk.free: every GPU test frees through it",
    "mgk_timer_create": "event timing (bench.py, the solver's walltime); no numerical result",
    "mgk_timer_start": "event timing (bench.py, the solver's walltime); no numerical result",
    "mgk_timer_stop": "event timing (bench.py, the solver's walltime); no numerical result",
    "mgk_timer_elapsed_ms": "event timing (bench.py, the solver's walltime); no numerical result",
    "mgk_timer_destroy": "event timing (bench.py, the solver's walltime); no numerical result",
    "mgk_stream_wait": "cross-stream ordering inside mg_solver.c / mg_comm.c, exercised by the slab and multi-rank solver tests",
    "mgk_capture_begin": "graph capture of the cycling loop in mg_solver.c, exercised by the solver tests",
    "mgk_capture_end": "graph capture of the cycling loop in mg_solver.c, exercised by the solver tests",
    "mgk_graph_launch": "graph replay in mg_solver.c, exercised by the solver tests",
    "mgk_graph_destroy": "graph teardown in mg_solver.c, exercised by the solver tests",
    "mgk_paced_copy": "the phantom transport's stand-in for link time (mg_comm.c), never on the product path",
    # profiling aids
    "mgk_debug_tail_stamps": "profiling aid (timestamps of the tail kernel's barriers, tools/tail_phases.py); off in production",
    "mgk_stream_triad_f64": "bandwidth probe of bench.py --full (STREAM triad); no result of the solver depends on it",
    # IPC and flag kernels of the peer halo transport: exercised through mg_comm.c by the transport tests
    "mgk_ipc_alloc": "peer transport (mg_comm.c), exercised by the multi-rank transport tests",
    "mgk_ipc_open": "peer transport (mg_comm.c), exercised by the multi-rank transport tests",
    "mgk_ipc_close": "peer transport (mg_comm.c), exercised by the multi-rank transport tests",
    "mgk_peer_copy": "peer transport (mg_comm.c), exercised by the multi-rank transport tests",
    "mgk_flags_set": "peer transport (mg_comm.c), exercised by the multi-rank transport tests",
    "mgk_flags_wait": "peer transport (mg_comm.c), exercised by the multi-rank transport tests",
    "mgk_flag_set": "peer transport (mg_comm.c), exercised by the multi-rank transport tests",
    "mgk_flag_wait": "peer transport (mg_comm.c), exercised by the multi-rank transport tests",
    "mgk_peer_allreduce": "peer transport's norm reduction (mg_comm.c), exercised by the multi-rank transport tests",
}


def _declared():
    with open(os.path.join(ROOT, "include", "mgk.h")) as f:
        h = f.read()
    return re.findall(r"^\s*(?:const\s+)?\w+\s*\**\s*(mgk_\w+)\s*\(", h, re.M)


def _test_text():
    text = []
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        if os.path.basename(p) != os.path.basename(__file__):
            with open(p) as f:
                text.append(f.read())
    return "\n".join(text)


def test_header_parses():
    names = _declared()
    assert len(names) == len(set(names)) > 100
    for n in ("mgk_geom_init", "mgk_csr_mult_f64", "mgk_tail_cycle_cs_f64", "mgk_ctx_destroy", "mgk_set_tuning", "mgk_last_error"):
        assert n in names


def test_every_kernel_entry_point_is_named_by_a_test():
    names = _declared()
    text = _test_text()
    gap = {n for n in names if not re.search(r"\b%s\b" % re.escape(n), text)}
    untested = sorted(gap - set(EXEMPT))
    assert not untested, f"entry points of include/mgk.h that no tests/test_*.py names (test them, or exempt them with a reason): {untested}"
    stale = sorted(set(EXEMPT) - gap)
    assert not stale, f"exempt entry points that a test now names or that the header no longer declares (drop the exemption): {stale}"


def test_every_exemption_has_a_reason():
    for name, why in EXEMPT.items():
        assert name.startswith("mgk_") and isinstance(why, str) and len(why.split()) >= 3, name
