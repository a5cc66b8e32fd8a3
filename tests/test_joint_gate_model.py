"""Joint compatibility gating without a GPU: the numpy model (tests/support/joint_gate_model.py) against its own contract -- prefixes,
permutation invariance, m = 1 against the single gate --, the open-chain scenario in which two candidates that each pass the single gate
contradict each other, and aprilsam_amd_marginals_set / aprilsam_amd_gate_xyt_joint as far as they go without a device: exported, the
argument refusals that precede the device, and -14 (there is no CPU fallback) with the outputs untouched."""
import subprocess
import sys

import numpy as np

from tests.conftest import ROOT
from tests.support.gate_model import CHI2_3_999, gate, gate_inputs, predict
from tests.support.joint_gate_model import dense_sigma, joint_gate, set_cov
from tests.support.marginal_cases import LAM, case_arrays
from tests.support.sigma_compare import ref_joint


def chain_scenario():
    """Open chain of 30 poses: unit steps in x, all headings 0, odometry W = diag(100, 100, 400), a 1e4 I prior on pose 0.  Two candidates
    between poses 2 and 29 with W = diag(400, 400, 1600): one at the prediction + (0, 1, 0), the other at the prediction - (0, 1, 0).
    Returns (arrays, a, b, z, W)."""
    N = 30
    states = np.c_[np.arange(N, dtype=float), np.zeros(N), np.zeros(N)]
    fa = np.r_[0, np.arange(N - 1)].astype(np.int32); fb = np.r_[-1, np.arange(1, N)].astype(np.int32)
    z = np.r_[[states[0]], np.tile([1.0, 0.0, 0.0], (N - 1, 1))]
    W = np.r_[[np.eye(3).ravel() * 1e4], np.tile(np.diag([100.0, 100.0, 400.0]).ravel(), (N - 1, 1))]
    a = np.array([2, 2], np.int32); b = np.array([29, 29], np.int32)
    pred = predict(states[2], states[29])
    zc = np.array([pred + [0, 1, 0], pred - [0, 1, 0]])
    Wc = np.tile(np.diag([400.0, 400.0, 1600.0]).ravel(), (2, 1))
    return (states, fa, fb, z, W), a, b, zc, Wc


def chi2_quantile(dof):
    from scipy.stats import chi2
    return chi2.ppf(0.999, dof)


def _case(lib, m, seed):
    arr = case_arrays(lib, "random1")
    Sig = dense_sigma(arr[0], *arr[1:], LAM)
    a, b, z, W = gate_inputs(arr, m, seed)
    z = np.array([predict(arr[0][i], arr[0][j]) for i, j in zip(a, b)]) + 0.2 * z      # (near the prediction: no residual on the wrap)
    return arr[0], Sig, a, b, z, W


def test_prefix_j_is_the_model_on_the_first_j_candidates(lib):
    st, Sig, a, b, z, W = _case(lib, 7, 1)
    a[3], b[3] = b[1], a[1]                                     # a repeated pair, the other way round
    a[5] = a[0]                                                 # a shared node
    pre, C, r = joint_gate(st, a, b, z, W, Sig)
    assert np.all(np.diff(pre) >= 0)
    for j in range(1, 8):
        pj, Cj, _ = joint_gate(st, a[:j], b[:j], z[:j], W[:j], Sig)
        assert abs(pj[-1] - pre[j - 1]) <= 1e-10 * pre[j - 1]
        assert np.abs(Cj - C[:3 * j, :3 * j]).max() <= 1e-13 * np.abs(C).max()      # (numpy's products: rounding only)


def test_total_is_permutation_invariant(lib):
    st, Sig, a, b, z, W = _case(lib, 9, 2)
    tot = joint_gate(st, a, b, z, W, Sig)[0][-1]
    rng = np.random.default_rng(0)
    for _ in range(5):
        k = rng.permutation(9)
        assert abs(joint_gate(st, a[k], b[k], z[k], W[k], Sig)[0][-1] - tot) <= 1e-10 * tot


def test_one_candidate_is_the_single_gate(lib):
    st, Sig, a, b, z, W = _case(lib, 12, 3)
    d2, S = gate(st, a, b, z, W, ref_joint(Sig, a, b))
    for i in range(12):
        pre, C, _ = joint_gate(st, a[i:i + 1], b[i:i + 1], z[i:i + 1], W[i:i + 1], Sig)
        assert abs(pre[0] - d2[i]) <= 1e-12 * d2[i] and np.abs(C - S[i]).max() <= 1e-12 * np.abs(S[i]).max()


def test_set_cov_repeats_the_blocks_of_a_repeated_node(lib):
    st, Sig, *_ = _case(lib, 1, 4)
    M = set_cov(Sig, [5, 2, 5])
    assert np.array_equal(M[:3, :3], M[6:, 6:]) and np.array_equal(M[:3, :3], M[:3, 6:]) and np.array_equal(M, M.T)
    assert np.array_equal(M[3:6, :3], Sig[6:9, 15:18])


def test_chain_scenario_two_passing_candidates_contradict_each_other():
    arr, a, b, z, W = chain_scenario()
    Sig = dense_sigma(arr[0], *arr[1:], LAM)
    single, _ = gate(arr[0], a, b, z, W, ref_joint(Sig, a, b))
    assert (single < CHI2_3_999).all() and np.allclose(single, 0.224, atol=1e-3)
    pre, C, r = joint_gate(arr[0], a, b, z, W, Sig)
    assert abs(pre[0] - single[0]) <= 1e-12 * single[0]
    dr = r[:3] - r[3:]
    Wi = [np.linalg.inv(w.reshape(3, 3)) for w in W]
    bound = dr @ np.linalg.solve(Wi[0] + Wi[1], dr)
    assert abs(bound - 800.0) < 1e-9
    assert pre[-1] > chi2_quantile(6) and pre[-1] >= bound * (1 - 1e-9)
    assert abs(pre[-1] - 800.0) < 0.5


NODEVICE = r"""
import sys; sys.path.insert(0, %r)
import ctypes as C
import numpy as np
from aprilsam_amd import abi, host, datasets
l = host.SolverLib()
for nm in ("aprilsam_amd_marginals_set", "aprilsam_amd_gate_xyt_joint"):
    assert hasattr(l.dll, nm), nm
assert abi.JOINT_MAX == 16
nodev = l.device_count() == 0
g = l.new_graph(); g.build_from_arrays(*datasets.random_pose_graph(5, 2, 0)); p = l.new_param()
ip, dp = host._np_i, host._np_d
W1 = np.diag([100.0, 100.0, 400.0]).ravel()

def joint(ptr, a, b, z=None, W=None, null=None):
    ptr = np.array(ptr, np.int32); a = np.array(a, np.int32); b = np.array(b, np.int32)
    n = len(a)
    z = np.zeros((n, 3)) if z is None else z
    W = np.tile(W1, (n, 1)) if W is None else W
    d2 = np.full(n + 1, -7.0); Cm = np.full(9 * 17 * 17, -7.0)
    args = [g.ptr, p.ptr, len(ptr) - 1, ip(ptr), ip(a), ip(b), dp(z), dp(W), dp(d2), dp(Cm)]
    if null is not None:
        args[null] = None
    l.clear_error()
    rc = l.dll.aprilsam_amd_gate_xyt_joint(*args)
    assert np.all(d2 == -7.0) and np.all(Cm == -7.0)
    assert rc == 0 or l.last_error()[0] == rc, (rc, l.last_error())
    return rc

# what precedes the device: -13 / -12 whatever the machine
for k in (0, 1, 3, 4, 5, 6, 7, 8):
    assert joint([0, 1], [0], [1], null=k) == -13, k
assert l.dll.aprilsam_amd_gate_xyt_joint(g.ptr, p.ptr, -1, None, None, None, None, None, None, None) == -13
assert joint([1, 2], [0, 0], [1, 1]) == -13                        # hyp_ptr does not start at 0
assert joint([0, 2, 1], [0, 0], [1, 1]) == -13                     # hyp_ptr decreases
assert joint([0, 0, 1], [0], [1]) == -13                           # an empty hypothesis
assert joint([0, 17], [0] * 17, [1] * 17) == -13                   # 17 candidates
assert joint([0, 16], [0] * 16, [1] * 16) != -13
assert joint([0, 2], [0, 3], [1, 3]) == -13                        # a == b
z = np.zeros((2, 3)); z[1, 2] = np.nan
assert joint([0, 2], [0, 2], [1, 3], z=z) == -13
W = np.tile(W1, (2, 1)); W[0, 8] = np.inf
assert joint([0, 2], [0, 2], [1, 3], W=W) == -13
W = np.tile(W1, (2, 1)); W[1, 1] += 0.5
assert joint([0, 2], [0, 2], [1, 3], W=W) == -12                   # asymmetric
W = np.tile(W1, (2, 1)); W[1] = np.diag([1.0, -1.0, 1.0]).ravel()
assert joint([0, 2], [0, 2], [1, 3], W=W) == -12                   # indefinite
cov = np.full(36, -7.0); nodes = np.array([0, 3], np.int32)
assert l.dll.aprilsam_amd_marginals_set(g.ptr, p.ptr, -1, ip(nodes), dp(cov)) == -13
assert l.dll.aprilsam_amd_marginals_set(g.ptr, p.ptr, 2, None, dp(cov)) == -13
assert l.dll.aprilsam_amd_marginals_set(g.ptr, p.ptr, 2, ip(nodes), None) == -13
assert l.dll.aprilsam_amd_marginals_set(g.ptr, None, 2, ip(nodes), dp(cov)) == -13
# well-formed calls: no device -14 (no CPU fallback); with one, a param that was never solved has no retained factor
want = -14 if nodev else -1
assert joint([0, 2, 3], [0, 2, 4], [1, 3, 0]) == want
assert joint([0], [], []) == want
for k in (0, 2):
    l.clear_error()
    assert l.dll.aprilsam_amd_marginals_set(g.ptr, p.ptr, k, ip(nodes), dp(cov)) == want
    assert l.last_error()[0] == want and np.all(cov == -7.0)
for call in (lambda: g.marginals_set(p, [0, 3]), lambda: g.gate_xyt_joint(p, [([0], [1], np.zeros((1, 3)), W1)])):
    try:
        call()
    except host.MarginalsError as e:
        assert e.code == want
    else:
        raise AssertionError("no error")
print("RETURNED")
"""


def test_entry_points_are_exported_and_refuse_in_order(built):
    """fails on a library without the two entry points"""
    r = subprocess.run([sys.executable, "-c", NODEVICE % ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RETURNED" in r.stdout, (r.stdout, r.stderr)
