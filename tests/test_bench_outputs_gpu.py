"""bench.py's plain run and --dump-outputs: the plain line carries the headline without the legs that moved behind --full, and the
dumped arrays are what the timed path computed -- the same solver driven directly (same configuration, the same warm-up and timed
cycles) yields the same residual history and the same solution."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_dumps_what_the_timed_path_computed(tmp_path):
    out = tmp_path / "out"
    steps, warmup, npts = 3, 1, 129
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--npts", str(npts), "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["steps"] == steps and j["warmup"] == warmup and j["ms_per_step"] > 0 and j["value"] > 0
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j
    for k in ("configs", "cpu_baseline", "history"):         # bench.py --full only
        assert k not in j
    assert "plain_sweep" not in j["roofline"] and "measured_ceiling" not in j["roofline"]

    rn = np.load(out / "residual_norms.npy")
    u = np.load(out / "solution_sample.npy")
    assert rn.dtype == np.float64 and u.dtype == np.float64
    assert rn.size == steps + warmup + 1
    assert u.size == (npts - 2) ** 3                         # below the sample budget: all of u

    from multigrid_petsc_amd.solver import Solver
    s = Solver(3, npts, 7, v=(3, 3), maxiter=steps + warmup + 1, scale=6.0 / 7.0, device=0)
    try:
        s.set_rhs_problem()
        s.cycles(warmup)
        s.cycles(steps)
        s.sync()
        want_rn, want_u = s.rnorm, s.solution()
    finally:
        s.close()
    assert np.max(np.abs(rn - want_rn) / want_rn) <= 1e-12
    assert np.array_equal(u, want_u)
