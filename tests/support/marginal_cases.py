"""Graphs the marginal-covariance tests share (tests/test_marginals_model.py, tests/test_gpu_marginals.py).  TEST-ONLY."""
import math

import numpy as np

from aprilsam_amd import datasets
from aprilsam_amd.harness import _xyt_inv_mul

LAM = 1e-4                       # april_graph_cholesky_param_init's tikhanov
RANDOM_SHAPES = ((12, 6), (80, 60), (400, 350), (1500, 900))       # tests/golden/random_<seed>.npz (tests/test_gpu_parity.py)


def tutorial_arrays():
    """the tutorial's final graph (aprilsam_amd/harness.run_tutorial): six poses on a line, a prior, odometry, one loop closure"""
    Wodo = np.diag([1.0 / 0.1 ** 2, 1.0 / 0.1 ** 2, 1.0 / math.radians(1) ** 2]).reshape(9)
    states = np.array([[k, 0.0, 0.0] for k in range(6)])
    fa, fb, z, W = [0], [-1], [[0.0, 0.0, 0.0]], [datasets.PRIOR_W]
    for k in range(1, 6):
        fa.append(k - 1); fb.append(k); z.append(_xyt_inv_mul([k - 1, 0, 0], [k, 0, 0])); W.append(Wodo)
    fa.append(0); fb.append(5); z.append(_xyt_inv_mul([0, 0, 0], [5, 1, 0])); W.append(Wodo)
    return states, np.array(fa, np.int32), np.array(fb, np.int32), np.array(z, float), np.array(W, float)


def case_arrays(lib, name):
    """'tutorial', 'random<seed>', 'lattice<K>', 'm3500'"""
    if name == "tutorial":
        return tutorial_arrays()
    if name.startswith("random"):
        seed = int(name[6:])
        return datasets.random_pose_graph(*RANDOM_SHAPES[seed], seed)
    if name.startswith("lattice"):
        return lib.lattice_arrays(int(name[7:]))
    if name == "m3500":
        return datasets.m3500_batch()
    raise ValueError(name)


def factor_pairs(fa, fb):
    """end poses of the binary factors"""
    fa = np.asarray(fa); fb = np.asarray(fb)
    m = fb >= 0
    return fa[m], fb[m]
