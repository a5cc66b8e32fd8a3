"""Joint covariances of any pose pair and gating, without a GPU: the numpy restatement of the path solves (tests/support/
pathsolve_model.py), driven by the library's own plan, against numpy's inverse of the same system for pairs on and off the pattern
of L; the gating model's Jacobians against finite differences; and the acceptance figures of the M3500 gating test
(tests/test_gpu_gating.py), derived here from the CPU reference solver."""
import numpy as np
import pytest

from tests.support.gate_model import CHI2_3_999, false_candidates, gate, held_out_closures, jacobians, predict
from tests.support.marginal_cases import LAM, case_arrays, factor_pairs
from tests.support.mf_emulator import PlanView
from tests.support.pathsolve_model import PathSolveModel
from tests.support.selinv_model import dense_system, sparse_system, system_blocks

MODEL_RTOL = 1e-9        # |model - inv(A)| / (largest entry of the two poses' block rows of inv(A))
GATE_ITERS = 10          # batch steps of the gating scenario (M3500 without its last 100 loop closures)
TRUE_ACCEPTED, FALSE_REJECTED = 100, 99        # of 100 held-out closures / 100 false candidates, at chi2_3(0.999)


def _pairs(N, rng, k=150):
    a = rng.integers(0, N, k).astype(np.int32); b = rng.integers(0, N, k).astype(np.int32)
    return np.r_[a, b, a[:10]], np.r_[b, a, a[:10]]              # both orders, and a == b


def _check(M, a, b, cols, scale):
    """cols(q): the three columns of inv(A) of node q"""
    J = M.joint_any(a, b)
    for k in range(len(a)):
        ca, cb = cols(a[k]), cols(b[k])
        ref = np.block([[ca[3 * a[k]:3 * a[k] + 3], cb[3 * a[k]:3 * a[k] + 3]], [ca[3 * b[k]:3 * b[k] + 3], cb[3 * b[k]:3 * b[k] + 3]]])
        e = np.abs(J[k] - ref).max() / max(scale(a[k]), scale(b[k]))
        assert e < MODEL_RTOL, (k, a[k], b[k], e)
    return J


@pytest.mark.parametrize("name", ["tutorial", "random0", "random1", "random2", "random3", "lattice6", "lattice24", "lattice40"])
def test_path_solves_equal_the_dense_inverse_for_any_pair(lib, name):
    states, fa, fb, z, W = case_arrays(lib, name)
    N = len(states)
    P = PlanView(lib, N, fa, fb, xy=states[:, :2])
    Aii, Aab = system_blocks(states, fa, fb, z, W, LAM)
    A = dense_system(Aii, Aab, fa, fb)
    Sig = np.linalg.inv(A)
    rowmax = np.abs(Sig).reshape(N, 3, 3 * N).max(axis=(1, 2))
    M = PathSolveModel(P, A)
    rng = np.random.default_rng(11)
    a, b = _pairs(N, rng)
    fa2, fb2 = factor_pairs(fa, fb)
    a, b = np.r_[a, fa2], np.r_[b, fb2]
    _check(M, a, b, lambda q: Sig[:, 3 * q:3 * q + 3], lambda q: rowmax[q])


def test_path_solves_on_m3500_with_held_out_closures(lib):
    """M3500 without its last 100 loop closures: the candidate pairs of those closures are (mostly) not on the pattern of L"""
    import scipy.sparse.linalg as sla
    arr = case_arrays(lib, "m3500")
    cl, (states, fa, fb, z, W) = held_out_closures(arr, 100)
    N = len(states)
    P = PlanView(lib, N, fa, fb, xy=states[:, :2])
    Aii, Aab = system_blocks(states, fa, fb, z, W, LAM)
    A = sparse_system(Aii, Aab, fa, fb).tocsc()
    M = PathSolveModel(P, A)
    rng = np.random.default_rng(12)
    a, b = _pairs(N, rng, 60)
    a, b = np.r_[arr[1][cl], a], np.r_[arr[2][cl], b]
    lu = sla.splu(A)
    nodes = np.unique(np.r_[a, b])
    E = np.zeros((3 * N, 3 * len(nodes)))
    for i, q in enumerate(nodes):
        E[3 * q:3 * q + 3, 3 * i:3 * i + 3] = np.eye(3)
    X = lu.solve(E)
    col = {int(q): X[:, 3 * i:3 * i + 3] for i, q in enumerate(nodes)}
    scale = {q: np.abs(c).max() for q, c in col.items()}
    _check(M, a, b, lambda q: col[int(q)], lambda q: scale[int(q)])
    # (the point of the feature: most of those pairs have their two poses in different fronts)
    apart = [M.path(int(x))[0] != M.path(int(y))[0] for x, y in zip(arr[1][cl], arr[2][cl])]
    assert sum(apart) > 50


def test_gate_model_jacobians_match_finite_differences():
    rng = np.random.default_rng(3)
    for _ in range(20):
        pa = rng.normal(size=3) * [5, 5, 2]; pb = rng.normal(size=3) * [5, 5, 2]
        z = predict(pa, pb) + rng.normal(size=3) * 0.1
        Ja, Jb, r = jacobians(pa, pb, z)
        h = 1e-6
        for k in range(3):
            e = np.zeros(3); e[k] = h
            da = (predict(pa + e, pb) - predict(pa - e, pb)) / (2 * h)
            db = (predict(pa, pb + e) - predict(pa, pb - e)) / (2 * h)
            assert np.abs(da - Ja[:, k]).max() < 1e-7 and np.abs(db - Jb[:, k]).max() < 1e-7
        zh = predict(pa, pb)
        assert np.allclose(r[:2], z[:2] - zh[:2]) and abs(np.cos(r[2]) - np.cos(z[2] - zh[2])) < 1e-12 and -np.pi <= r[2] < np.pi


def m3500_gate_scenario(oracle_or_states, lp=None):
    """the candidates of the gating test and, from the given solution (states, lp), the model's d2"""
    import scipy.sparse.linalg as sla
    from aprilsam_amd import datasets
    arr = datasets.m3500_batch()
    cl, ho = held_out_closures(arr, 100)
    fa_, fb_, fz, fW = false_candidates(arr, cl, 100)
    a = np.r_[arr[1][cl], fa_].astype(np.int32); b = np.r_[arr[2][cl], fb_].astype(np.int32)
    z = np.r_[arr[3][cl], fz]; W = np.r_[arr[4][cl], fW]
    if lp is None:
        return ho, a, b, z, W
    st = oracle_or_states
    Aii, Aab = system_blocks(lp, ho[1], ho[2], ho[3], ho[4], LAM)
    lu = sla.splu(sparse_system(Aii, Aab, ho[1], ho[2]).tocsc())
    nodes = np.unique(np.r_[a, b])
    E = np.zeros((3 * len(st), 3 * len(nodes)))
    for i, q in enumerate(nodes):
        E[3 * q:3 * q + 3, 3 * i:3 * i + 3] = np.eye(3)
    X = lu.solve(E)
    ci = {int(q): i for i, q in enumerate(nodes)}
    J = np.empty((len(a), 6, 6))
    for k in range(len(a)):
        ix = np.r_[3 * a[k]:3 * a[k] + 3, 3 * b[k]:3 * b[k] + 3]
        J[k] = np.hstack([X[ix, 3 * ci[int(a[k])]:3 * ci[int(a[k])] + 3], X[ix, 3 * ci[int(b[k])]:3 * ci[int(b[k])] + 3]])
    d2, S = gate(st, a, b, z, W, J)
    return d2, S, J


def test_m3500_gate_rates_on_the_cpu(oracle):
    """the figures tests/test_gpu_gating.py asserts: the CPU reference solver's solution, the model's gate"""
    ho, a, b, z, W = m3500_gate_scenario(None)
    _, lp = oracle.iterate(ho, GATE_ITERS - 1)
    _, st = oracle.iterate(ho, GATE_ITERS)
    d2, _, _ = m3500_gate_scenario(st, lp)
    acc = d2 < CHI2_3_999
    assert int(acc[:100].sum()) == TRUE_ACCEPTED and int((~acc[100:]).sum()) == FALSE_REJECTED
    assert np.abs(np.log(d2 / CHI2_3_999)).min() > 0.3          # (no candidate near the gate: the GPU's decisions cannot flip on rounding)
