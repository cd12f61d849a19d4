"""GPU tier: whole solver sessions drawn at random (fixed seeds) -- one Solver and a sequence of operations on the same live handle (new
right-hand sides, reset, solve, the bench's fixed-count loop, fmg, solve_fmg, solve_gmres on point Jacobi; solve and the fixed-count loop on
the y-line / x-line / alternating line smoothers with line_chunk / xline_chunk, with the refusals of fmg / solve_fmg / solve_gmres), every
result compared with a reference that starts afresh: iterations equal, u bit-identical, the history to 1e-10 (GMRES: the bars of
tests/test_gmres_cpu.py).  tools/stress_sessions.py runs the draw of tools/stress_sessions_mock.py over the real libraries with the larger
sizes (point 2-D npts 9 .. 1025, 3-D 9 .. 129; line 9 .. 257); tests/test_random_sessions_cpu.py is the CPU tier.  Neither test reads the
reference tree or oracle/_ref/.

Counts, seeds and wall times of the child process (the references on the host included), measured once on the MI355X:
  point  40 sessions, seed 11:  4 s   (2-D up to 1025 three times, 3-D 129 three times; 62 right-hand sides, 38 fmg, 22 solve_fmg, 2 solve_gmres)
  line   30 sessions, seed 5:   6 s   (npts 257 five times; 40 cycles legs, 27 solves, 1 refusal)
Far inside the minute a test may take: the counts are the ones the draw was introduced with and can grow."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(kind, count, seed, timeout):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stress_sessions.py"), str(count), str(seed), kind], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0 and f"{count} sessions, 0 mismatches, 0 refused" in p.stdout, p.stdout[-4000:]
    assert "MISMATCH" not in p.stdout and "REFUSED" not in p.stdout, p.stdout[-4000:]


@pytest.mark.timeout(600)
def test_random_point_jacobi_sessions_equal_their_references():
    _run("point", 40, 11, 500)


@pytest.mark.timeout(600)
def test_random_line_smoother_sessions_equal_their_references():
    _run("line", 30, 5, 500)
