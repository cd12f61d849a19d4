"""numpy statement of the 2-D row-table operators (the reference's stretched meshes, -mesh 1/2): per grid row i five coefficients
{(i-1), W, C, E, (i+1)}, terms summed in that order (include/mgk.h, mgk_rowcoef_f64).  Shared by the GPU tests that pin the
row-table kernels."""
import numpy as np


def _rt_apply(ct, u):
    """A u for the row-table operator: per grid row i the five coefficients {(i-1), W, C, E, (i+1)}, terms summed in that order"""
    n = u.shape[0]
    p = np.zeros((n + 2, n + 2))
    p[1:-1, 1:-1] = u
    t = ct[:, 0:1] * p[:-2, 1:-1]
    t = t + ct[:, 1:2] * p[1:-1, :-2]
    t = t + ct[:, 2:3] * p[1:-1, 1:-1]
    t = t + ct[:, 3:4] * p[1:-1, 2:]
    t = t + ct[:, 4:5] * p[2:, 1:-1]
    return t


def _rt_jacobi(ct, b, u, scale):
    res = b - _rt_apply(ct, u)
    return u + scale * (res * (1.0 / ct[:, 2:3]))


def _rt_tables(rng, n):
    q = float((n + 1) ** 2)
    ct = np.empty((n, 5))
    ct[:, 0] = q * rng.uniform(0.5, 1.5, n)
    ct[:, 1] = q * rng.uniform(0.5, 1.5, n)
    ct[:, 3] = ct[:, 1]
    ct[:, 4] = q * rng.uniform(0.5, 1.5, n)
    ct[:, 2] = -(ct[:, 0] + ct[:, 1] + ct[:, 3] + ct[:, 4])
    return ct, 1.0 / ct[:, 2]
