"""Solves with the retained factor, without a GPU: the numpy restatement of the two whole-tree passes (tests/support/treesolve_model.py),
driven by the library's own plan, against numpy's dense solve and inverse of the same system; the relative-covariance model against
the gating model; and the calibration of the backward-error limit of tests/test_gpu_treesolve.py on the lattices (scipy's splu)."""
import numpy as np
import pytest

from tests.support.gate_model import gate
from tests.support.marginal_cases import LAM, case_arrays
from tests.support.mf_emulator import PlanView
from tests.support.selinv_model import dense_system, sparse_system, system_blocks
from tests.support.treesolve_model import (BACKWARD, FORWARD, FULL, LATTICE_OMEGA_LIMIT, OMEGA_LIMIT, TreeSolveModel, backward_error,
                                           relative_covariances, rhs_columns)

MODEL_RTOL = 1e-9        # |model - reference| / (largest entry of the reference), as tests/test_pathsolve_model.py


def _rel(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("name", ["tutorial", "random0", "random1", "random2", "random3", "lattice6", "lattice24"])
def test_tree_solves_equal_the_dense_solve_and_inverse(lib, name):
    states, fa, fb, z, W = case_arrays(lib, name)
    N = len(states)
    P = PlanView(lib, N, fa, fb, xy=states[:, :2])
    Aii, Aab = system_blocks(states, fa, fb, z, W, LAM)
    A = dense_system(Aii, Aab, fa, fb)
    Sig = np.linalg.inv(A)
    M = TreeSolveModel(P, A)
    rng = np.random.default_rng(5)
    B = rng.normal(size=(3 * N, 7))
    B[:, 3] = 0.0
    X = M.solve(B, FULL)
    assert _rel(X, np.linalg.solve(A, B)) < MODEL_RTOL
    assert np.all(X[:, 3] == 0.0)
    assert backward_error(A, X, B).max() < OMEGA_LIMIT
    Y = M.solve(B, FORWARD)
    assert _rel(M.solve(Y, BACKWARD), X) < 1e-13             # BACKWARD o FORWARD is FULL (the same operations)
    # the half-solves of the identity: both Gram matrices are Sigma
    I = np.eye(3 * N)
    Fw, Bw = M.solve(I, FORWARD), M.solve(I, BACKWARD)
    assert _rel(Fw.T @ Fw, Sig) < MODEL_RTOL
    assert _rel(Bw @ Bw.T, Sig) < MODEL_RTOL
    # cross blocks with an anchor: first, middle, last node and a pose of the root front
    for anchor in (0, N // 2, N - 1, int(P.perm[-1])):
        C = M.cross(anchor)
        ref = Sig[:, 3 * anchor:3 * anchor + 3].reshape(N, 3, 3)
        assert _rel(C, ref) < MODEL_RTOL, anchor
    sub = rng.integers(0, N, 5)
    assert np.array_equal(M.cross(1, sub), M.cross(1)[sub])


@pytest.mark.parametrize("name", ["random1", "random2"])
def test_relative_covariances_equal_the_gate_models_s_minus_w_inverse(lib, name):
    """states differ from the linearisation points: Sigma at the l_points, Jacobians at the states"""
    lp, fa, fb, z, W = case_arrays(lib, name)
    N = len(lp)
    rng = np.random.default_rng(9)
    states = lp + rng.normal(size=lp.shape) * [0.05, 0.05, 0.02]
    Aii, Aab = system_blocks(lp, fa, fb, z, W, LAM)
    A = dense_system(Aii, Aab, fa, fb)
    Sig = np.linalg.inv(A)
    P = PlanView(lib, N, fa, fb, xy=lp[:, :2])
    M = TreeSolveModel(P, A)
    anchor = N - 1
    nodes = np.arange(N)
    Sia = M.cross(anchor)
    Sii = np.array([Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in nodes])
    Saa = Sig[3 * anchor:3 * anchor + 3, 3 * anchor:3 * anchor + 3]
    R = relative_covariances(states, anchor, nodes, Saa, Sii, Sia)
    others = nodes[nodes != anchor]
    a = np.full(len(others), anchor)
    joint = np.empty((len(others), 6, 6))
    for k, i in enumerate(others):
        ix = np.r_[3 * anchor:3 * anchor + 3, 3 * i:3 * i + 3]
        joint[k] = Sig[np.ix_(ix, ix)]
    Wg = np.tile(np.eye(3).reshape(9), (len(others), 1))
    _, S = gate(states, a, others, np.zeros((len(others), 3)), Wg, joint)
    ref = S - np.eye(3)
    for k, i in enumerate(others):
        assert np.abs(R[i] - ref[k]).max() < MODEL_RTOL * np.abs(ref[k]).max(), i
    assert np.all(R[anchor] == 0.0)


@pytest.mark.parametrize("K,nrhs", [(60, 17), (316, 3)])
def test_backward_error_of_a_cpu_sparse_solve_on_the_lattices(lib, K, nrhs):
    """What the lattice limits of tests/test_gpu_treesolve.py rest on: the backward error scipy's splu reaches on the same system and
    right-hand sides.  Printed; the limit is 1e-12, or 100 x this figure where that is larger (LATTICE_OMEGA_LIMIT)."""
    import scipy.sparse.linalg as sla
    states, fa, fb, z, W = case_arrays(lib, f"lattice{K}")
    N = len(states)
    Aii, Aab = system_blocks(states, fa, fb, z, W, LAM)
    A = sparse_system(Aii, Aab, fa, fb).tocsc()
    B = rhs_columns(N, nrhs, K)
    X = sla.splu(A).solve(B)
    w = backward_error(A, X, B).max()
    print(f"lattice K = {K}, nrhs = {nrhs}: splu backward error {w:.3e}; GPU limit {LATTICE_OMEGA_LIMIT[K]:.3e}")
    assert w < OMEGA_LIMIT
    # the recorded limit is max(1e-12, 100 x this figure), to the two digits it is written with (and to splu's build-to-build spread)
    basis = max(OMEGA_LIMIT, 100 * w)
    assert 0.8 * basis <= LATTICE_OMEGA_LIMIT[K] <= 1.25 * basis, (LATTICE_OMEGA_LIMIT[K], basis)
