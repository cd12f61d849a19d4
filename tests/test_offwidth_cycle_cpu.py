"""CPU tier of tests/test_offwidth_cycle_gpu.py: the point-Jacobi cases of tests/offwidth_cases.py (3-D fp64 and mixed precision under the default
fusions, fuse=0 and pair_min_n=7; 2-D on meshes 0, 1, 2 under Richardson and Chebyshev; 2 and 3 loopback slab ranks) with the product's host logic
over the host stand-in of the kernel ABI, at the small sizes: npts 13, 25 and 49 in 3-D, 49 and 97 in 2-D.  What it can find is what the host decides
at these widths: the depth check of mg_solver_create, which pass runs on which level, the slab split of a width that is no power of two.  (The line
smoothers, red-black Gauss-Seidel, FMG and GMRES have stand-in libraries of their own, tests/test_*line*_cpu.py and the like; their off-width cases run
in the GPU tier.)  And the draws of tools/stress_solver_mock.py with its off-width size lists, one fixed seed."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.timeout(900)
def test_off_width_solves_on_the_host_mock_equal_the_oracle():
    p = subprocess.run([sys.executable, os.path.join(HERE, "offwidth_mock_worker.py"), "13,25,49", "49,97", "25"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=800, cwd=ROOT)
    assert p.returncode == 0 and "offwidth mock: 38 cases, 0 mismatches" in p.stdout, p.stdout[-3000:]


@pytest.mark.timeout(600)
def test_random_off_width_configurations_on_the_host_mock_equal_the_oracle():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stress_solver_mock.py"), "80", "303", "problem", "offwidth"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=500, cwd=ROOT)
    assert p.returncode == 0 and "80 configurations, 0 mismatches" in p.stdout, p.stdout[-3000:]
    assert "REFUSED" not in p.stdout, p.stdout[-3000:]
