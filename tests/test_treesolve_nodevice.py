"""aprilsam_amd_solve / aprilsam_amd_marginals_cross / aprilsam_amd_relative_covariances on a machine without a HIP device: exported,
and -- there being no CPU fallback -- refused with -14, the error recorded and the outputs untouched."""
import subprocess
import sys

import pytest

from tests.conftest import ROOT

CODE = r"""
import sys; sys.path.insert(0, %r)
import ctypes as C
import numpy as np
from aprilsam_amd import host, datasets
l = host.SolverLib()
for nm in ("aprilsam_amd_solve", "aprilsam_amd_marginals_cross", "aprilsam_amd_relative_covariances", "aprilsam_amd_debug_solve_bytes",
           "aprilsam_amd_factorised_nodes"):
    assert hasattr(l.dll, nm), nm
g = l.new_graph(); g.build_from_arrays(*datasets.random_pose_graph(5, 2, 0)); p = l.new_param()
B = np.arange(30.0); X = np.full(30, -7.0)
for mode in (0, 1, 2):
    l.clear_error()
    assert l.dll.aprilsam_amd_solve(g.ptr, p.ptr, mode, 2, B.ctypes.data_as(host._dp), X.ctypes.data_as(host._dp)) == -14
    assert l.last_error()[0] == -14 and np.all(X == -7.0)
cov = np.full(45, -7.0); nodes = np.array([0, 3], np.int32)
for fn in (l.dll.aprilsam_amd_marginals_cross, l.dll.aprilsam_amd_relative_covariances):
    for n, q in ((0, None), (2, nodes.ctypes.data_as(host._ip))):
        l.clear_error()
        assert fn(g.ptr, p.ptr, 1, n, q, cov.ctypes.data_as(host._dp)) == -14
        assert l.last_error()[0] == -14 and np.all(cov == -7.0)
for call in (lambda: g.solve(p, B.reshape(2, 15)), lambda: g.marginals_cross(p, 0), lambda: g.relative_covariances(p, 0, [1, 2])):
    try:
        call()
    except host.MarginalsError as e:
        assert e.code == -14
    else:
        raise AssertionError("no error")
assert l.dll.aprilsam_amd_debug_solve_bytes(p.ptr) == -1 and l.dll.aprilsam_amd_factorised_nodes(p.ptr) == -1
print("RETURNED")
"""


def test_solve_entry_points_refuse_without_a_device(lib):
    if lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    r = subprocess.run([sys.executable, "-c", CODE % ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RETURNED" in r.stdout, (r.stdout, r.stderr)
