"""The numpy model of the information measures (tests/support/info_model.py) against independent truths, on the CPU:
logdet against slogdet and an extended-precision Cholesky, the gain against the determinant lemma by really adding the factors, a set of
all nodes against -logdet, zero mutual information across components, and the sensitivity controls that show the GPU test's tolerance can
tell a wrong diagonal address from rounding."""
import numpy as np
import pytest

from tests.support import info_model as IM
from tests.support.consumer_graphs import two_components
from tests.support.joint_gate_model import innovation_rows
from tests.support.marginal_cases import LAM, case_arrays
from tests.support.sigma_compare import SIG_RTOL

CASES = ["tutorial", "random0", "random1", "random2", "random3"]


@pytest.fixture(scope="module")
def systems(lib):
    """per case: arrays, A at the graph's own states, its inverse, the model's logdet and its tolerance -- computed once"""
    out = {}
    for name in CASES:
        arr = case_arrays(lib, name)
        A = IM.system_matrix(arr[0], *arr[1:], LAM)
        out[name] = dict(arr=arr, A=A, Sig=np.linalg.inv(A), ld=IM.logdet(A), tol=IM.logdet_tolerance(A))
    return out


def _longdouble_logdet(A):
    n = len(A)
    M = A.astype(np.longdouble); L = np.zeros((n, n), np.longdouble)
    for c in range(n):
        L[c, c] = np.sqrt(M[c, c] - L[c, :c] @ L[c, :c])
        L[c + 1:, c] = (M[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
    return float(2 * np.log(np.diag(L)).sum())


@pytest.mark.parametrize("name", CASES)
def test_logdet_against_slogdet_and_extended_precision(systems, name):
    s = systems[name]
    sign, ref = np.linalg.slogdet(s["A"])
    print(f"{name}: logdet {s['ld']:.12g}, slogdet differs by {abs(s['ld'] - ref):.2e}, tolerance {s['tol']:.2e}")
    assert sign == 1 and abs(s["ld"] - ref) <= 2 * s["tol"]          # (the LU behind slogdet rounds as much as the Cholesky does)
    if len(s["arr"][0]) <= 40:
        assert abs(s["ld"] - _longdouble_logdet(s["A"])) <= s["tol"]


def _hypothesis(N, m, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N, m); b = (a + rng.integers(1, N, m)) % N
    if m >= 3:
        a[2], b[2] = b[0], a[0]                                  # a pair again, the other way round
    L = rng.normal(size=(m, 3, 3)) * 0.3 + np.eye(3) * 3
    return a.astype(np.int32), b.astype(np.int32), np.einsum("nij,nkj->nik", L, L)


@pytest.mark.parametrize("name", CASES)
def test_gain_is_the_growth_of_logdet_when_the_factors_are_added(systems, name):
    s = systems[name]
    st = s["arr"][0]
    N = len(st)
    for m in (1, 2, 5, 16):
        a, b, W = _hypothesis(N, m, 10 * m + N)
        pre = IM.gain_prefixes(st, a, b, W, s["Sig"])
        assert (pre >= 0).all() and (np.diff(pre) >= 0).all()
        loose = IM.gain_loose_tolerance(st, a, b, W, s["Sig"], SIG_RTOL)
        for j in range(m):
            H, _ = innovation_rows(st, a[:j + 1], b[:j + 1], np.zeros((j + 1, 3)), 3 * N)
            ref = IM.gain_by_adding(s["A"], H, W[:j + 1])
            assert abs(pre[j] - ref) <= s["tol"] + loose[j], (name, m, j, pre[j], ref)


@pytest.mark.parametrize("name", ["tutorial", "random0"])
def test_the_set_of_all_nodes_gives_minus_logdet(systems, name):
    s = systems[name]
    N = len(s["arr"][0])
    assert N <= 16
    nodes = np.random.default_rng(N).permutation(N)
    pre = IM.set_prefixes(s["Sig"], nodes)
    M = IM.set_cov(s["Sig"], nodes)
    assert abs(pre[-1] + s["ld"]) <= s["tol"] + IM.set_tight_tolerance(M)[-1] + IM.set_loose_tolerance(M, s["Sig"], nodes, SIG_RTOL)[-1]
    assert np.isfinite(pre).all()


def test_mutual_information_across_components_is_zero():
    arr, comp = two_components()
    Sig = np.linalg.inv(IM.system_matrix(arr[0], *arr[1:], LAM))
    n0 = np.nonzero(comp == 0)[0]; n1 = np.nonzero(comp == 1)[0]
    A, B = n0[[0, 7, 200, 399]], n1[[3, 50, 79]]
    AB = np.r_[A, B]
    lA, lB, lAB = (IM.set_prefixes(Sig, x)[-1] for x in (A, B, AB))
    tol = sum(IM.set_tight_tolerance(IM.set_cov(Sig, x))[-1] for x in (A, B, AB))
    mi = 0.5 * (lA + lB - lAB)
    print(f"mutual information across components {mi:.3e}, tolerance {tol:.3e}")
    assert abs(mi) <= tol
    inside = 0.5 * (IM.set_prefixes(Sig, A[:2])[-1] + IM.set_prefixes(Sig, A[2:])[-1] - IM.set_prefixes(Sig, A)[-1])
    assert inside > 1e3 * tol                                    # (within a component there is some)


def test_a_set_with_a_fixed_node_is_nan_from_that_node_on(systems):
    s = systems["random1"]
    from tests.support.joint_gate_model import dense_sigma
    arr = s["arr"]
    Sig = dense_sigma(arr[0], *arr[1:], LAM, None, (7,))
    pre = IM.set_prefixes(Sig, [3, 7, 9])
    assert np.isfinite(pre[0]) and np.isnan(pre[1:]).all()
    assert abs(IM.logdet(s["A"], (7,)) - np.linalg.slogdet(IM.free_block(s["A"], (7,)))[1]) <= 2 * s["tol"]


@pytest.mark.parametrize("name", CASES)
def test_sensitivity_controls(systems, name):
    """what the GPU test is meant to catch moves the value by more than its tolerance: a front's diagonal left out (here the smallest
    front there is, one pose: every pose in turn), and a diagonal read one row too low (every column in turn)"""
    s = systems[name]
    L = np.linalg.cholesky(s["A"])
    n = len(L)
    skip = min(abs(IM.logdet_of_factor(L, skip=range(3 * i, 3 * i + 3)) - s["ld"]) for i in range(n // 3))
    with np.errstate(divide="ignore"):
        low = min(abs(IM.logdet_of_factor(L, lower=j) - s["ld"]) for j in range(n - 1))
    print(f"{name}: tolerance {s['tol']:.2e}; a pose left out moves logdet by >= {skip:.2e}, a diagonal read one row low by >= {low:.2e}")
    assert skip > s["tol"] and low > s["tol"]
