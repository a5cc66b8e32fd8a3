"""Marginal covariances without a GPU: the numpy restatement of the selected inversion (tests/support/selinv_model.py), driven by
the library's own plan, against numpy's inverse of the same system; the matrix-free identity checker the GPU tests use
(tests/support/marginal_identity.py) with its negative control; and the entry points' refusal on a box without a device."""
import numpy as np
import pytest

from tests.support.marginal_cases import LAM, case_arrays, factor_pairs
from tests.support.marginal_identity import identity_residual
from tests.support.mf_emulator import PlanView
from tests.support.selinv_model import SelInvModel, dense_system, sparse_system, system_blocks

MODEL_RTOL = 1e-9        # |model - inv(A)| / (largest entry of the block row of inv(A)); observed <= 2e-12 (lattice 40)


def _model(lib, arr):
    states, fa, fb, z, W = arr
    P = PlanView(lib, len(states), fa, fb, xy=states[:, :2])
    Aii, Aab = system_blocks(states, fa, fb, z, W, LAM)
    return P, Aii, Aab


def _block_row_scale(Sig, N):
    """per pose: the largest |entry| of its three rows of Sigma"""
    return np.abs(Sig).reshape(N, 3, 3 * N).max(axis=(1, 2))


@pytest.mark.parametrize("name", ["tutorial", "random0", "random1", "random2", "random3", "lattice6", "lattice24", "lattice40"])
def test_model_equals_the_dense_inverse_on_the_pattern(lib, name):
    arr = case_arrays(lib, name)
    states, fa, fb = arr[0], arr[1], arr[2]
    N = len(states)
    P, Aii, Aab = _model(lib, arr)
    A = dense_system(Aii, Aab, fa, fb)
    Sig = np.linalg.inv(A)
    M = SelInvModel(P, A)
    scale = _block_row_scale(Sig, N)
    diag = M.marginals()
    ref = np.stack([Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(N)])
    err = np.abs(diag - ref).reshape(N, 9).max(axis=1) / scale
    assert err.max() < MODEL_RTOL, err.max()
    a, b = factor_pairs(fa, fb)
    J = M.joint(a, b)
    assert not np.isnan(J).any(), "a factor pair off the pattern of L"
    if N > 40:      # pairs of all poses: those the lookup finds are Sigma's blocks, the others all NaN (both orders of elimination)
        qa, qb = np.meshgrid(np.arange(0, N, 7), np.arange(3, N, 11))
        qa, qb = qa.ravel(), qb.ravel()
        Jq = M.joint(qa, qb)
        offp = np.isnan(Jq).any(axis=(1, 2))
        assert (np.isnan(Jq[offp]).all() and (offp & (M.pos[qa] < M.pos[qb])).any() and (offp & (M.pos[qa] > M.pos[qb])).any())
        for k in np.nonzero(~offp)[0]:
            ix = np.r_[3 * qa[k]:3 * qa[k] + 3, 3 * qb[k]:3 * qb[k] + 3]
            assert np.abs(Jq[k] - Sig[np.ix_(ix, ix)]).max() < MODEL_RTOL * max(scale[qa[k]], scale[qb[k]])
    for k in range(len(a)):
        ix = np.r_[3 * a[k]:3 * a[k] + 3, 3 * b[k]:3 * b[k] + 3]
        e = np.abs(J[k] - Sig[np.ix_(ix, ix)]).max() / max(scale[a[k]], scale[b[k]])
        assert e < MODEL_RTOL, (k, e)


def test_model_on_the_60x60_lattice_satisfies_the_identity_and_matches_sparse_solves(lib):
    import scipy.sparse.linalg as sla
    arr = case_arrays(lib, "lattice60")
    states, fa, fb = arr[0], arr[1], arr[2]
    N = len(states)
    P, Aii, Aab = _model(lib, arr)
    A = sparse_system(Aii, Aab, fa, fb)
    M = SelInvModel(P, A)
    a, b = factor_pairs(fa, fb)
    jf = np.zeros((len(fa), 6, 6)); jf[fb >= 0] = M.joint(a, b)
    res = identity_residual(Aii, Aab, fa, fb, M.marginals(), jf)
    assert res["rel_max"] < 1e-12, res["rel_max"]
    lu = sla.splu(A.tocsc())
    for i in np.random.default_rng(0).choice(N, 8, replace=False):
        E = np.zeros((3 * N, 3)); E[3 * i:3 * i + 3] = np.eye(3)
        col = lu.solve(E)
        assert np.abs(M.marginals([i])[0] - col[3 * i:3 * i + 3]).max() < MODEL_RTOL * np.abs(col).max()


@pytest.mark.parametrize("name", ["random2", "lattice24"])
def test_identity_checker_is_at_rounding_for_the_inverse_and_order_one_for_a_wrong_sigma(lib, name):
    arr = case_arrays(lib, name)
    states, fa, fb = arr[0], arr[1], arr[2]
    N = len(states)
    _, Aii, Aab = _model(lib, arr)
    Sig = np.linalg.inv(dense_system(Aii, Aab, fa, fb))
    diag = np.stack([Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(N)])
    joint = np.zeros((len(fa), 6, 6))
    for k in range(len(fa)):
        if fb[k] >= 0:
            ix = np.r_[3 * fa[k]:3 * fa[k] + 3, 3 * fb[k]:3 * fb[k] + 3]
            joint[k] = Sig[np.ix_(ix, ix)]
    good = identity_residual(Aii, Aab, fa, fb, diag, joint)
    assert good["rel_max"] < 1e-11, good["rel_max"]
    # negative controls: one pose's diagonal block 1 % off -> that pose's residual, and only its, leaves rounding; the cross blocks of
    # every factor pair lost (what a missing gather from the parent front would leave) -> order one
    k = N // 2
    bad = diag.copy(); bad[k] *= 1.01
    r = identity_residual(Aii, Aab, fa, fb, bad, joint)
    assert r["rel_per_pose"][k] > 1e-4 and np.delete(r["rel_per_pose"], k).max() < 1e-11
    nocross = joint.copy(); nocross[:, :3, 3:] = 0; nocross[:, 3:, :3] = 0
    assert identity_residual(Aii, Aab, fa, fb, diag, nocross)["rel_max"] > 0.1


def test_marginals_refuse_without_a_device(lib):
    """No CPU fallback: both entry points return -14 and record it; the param stays usable (the next call says the same)."""
    if lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    import subprocess, sys
    from tests.conftest import ROOT
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from aprilsam_amd import host, datasets\n"
            "l = host.SolverLib(); g = l.new_graph(); g.build_from_arrays(*datasets.random_pose_graph(5, 2, 0)); p = l.new_param()\n"
            "out = np.zeros(9 * 5)\n"
            "assert l.dll.aprilsam_amd_marginals(g.ptr, p.ptr, 0, None, out.ctypes.data_as(host._dp)) == -14\n"
            "assert l.last_error()[0] == -14\n"
            "a = np.array([0, 1], np.int32); b = np.array([1, 2], np.int32); j = np.zeros(72)\n"
            "assert l.dll.aprilsam_amd_marginals_joint(g.ptr, p.ptr, 2, a.ctypes.data_as(host._ip), b.ctypes.data_as(host._ip), j.ctypes.data_as(host._dp)) == -14\n"
            "try:\n    g.marginals(p)\nexcept host.MarginalsError as e:\n    assert e.code == -14\nelse:\n    raise AssertionError('no error')\n"
            "g.cholesky(p); assert l.last_error()[0] == -14\n"
            "assert l.dll.aprilsam_amd_marginals(g.ptr, p.ptr, 0, None, out.ctypes.data_as(host._dp)) == -14\n"
            "print('RETURNED')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RETURNED" in r.stdout, (r.stdout, r.stderr)
