#!/usr/bin/env python3
"""Whole solver sessions drawn at random against their references on the GPU (a one-off stress run; a fixed-seed share of it is in the GPU suite,
tests/test_random_sessions_gpu.py): one Solver and a sequence of operations on the same live handle -- new right-hand sides, reset, solve, the
bench's fixed-count loop, fmg, solve_fmg, solve_gmres (point Jacobi), or the line smoothers with line_chunk / xline_chunk -- every result
compared with a reference that starts afresh: iterations equal, u bit-identical, the history to 1e-10.  The draw and the comparison live in
tools/stress_sessions_mock.py, which runs them on the CPU over the host mock with the small sizes.  Here: point 2-D npts 9 .. 1025, 3-D
9 .. 129; line npts 9 .. 257 -- the smallest sizes that put levels above the LDS tail: the levels of 127 and 255 (2-D) and 31 and 63 (3-D) are
what the FMG interpolation pass, the recorded coarse-level graph and the chunked line sweeps run on.  The numpy line references, not the GPU,
set the time on the line side.  mgk_interp_jacobi2_f64 is built for rows of 512 / 1024 alone (a 513^3 grid and larger): it stays with
tests/test_fmg_gpu.py and is out of this draw's reach.  usage: stress_sessions.py [count] [seed] [point|line] [only]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stress_sessions_mock import main

if __name__ == "__main__":
    main(mock=False)
