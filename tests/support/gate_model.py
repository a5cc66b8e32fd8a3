"""numpy model of aprilsam_amd_gate_xyt (k_gate_xyt, aprilsam_amd/csrc/pathsolve.hip.h).  TEST-ONLY.

For a candidate xyt measurement z with information W between poses a and b:
    r, J_a, J_b    the xyt factor's residual z - pa^-1 o pb (theta wrapped) and the Jacobians of the prediction, at the states
    S  = [J_a J_b] Sigma_ab [J_a J_b]' + W^-1      (Sigma_ab: the 6 x 6 joint covariance, at the linearisation points)
    d2 = r' S^-1 r
"""
import numpy as np

from .normal_eq import linearise

CHI2_3_999 = 16.266236196238129      # chi^2 with 3 degrees of freedom, 0.999 quantile


def predict(pa, pb):
    """the xyt prediction pa^-1 o pb"""
    ca, sa = np.cos(pa[2]), np.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    return np.array([ca * dx + sa * dy, -sa * dx + ca * dy, pb[2] - pa[2]])


def jacobians(pa, pb, z):
    """J_a, J_b (3 x 3 each) and r, as the library's xyt factor computes them"""
    st = np.array([pa, pb], float)
    Ja, Jb, r = linearise(st, np.array([0]), np.array([1]), np.asarray(z, float).reshape(1, 3))
    return Ja[0], Jb[0], r[0]


def gate(states, a, b, z, W, joint):
    """d2 [n], S [n, 3, 3]; joint [n, 6, 6]"""
    states = np.asarray(states, float)
    n = len(a)
    d2 = np.empty(n); S = np.empty((n, 3, 3))
    for i in range(n):
        Ja, Jb, r = jacobians(states[a[i]], states[b[i]], z[i])
        J = np.hstack([Ja, Jb])
        S[i] = J @ joint[i] @ J.T + np.linalg.inv(np.asarray(W[i], float).reshape(3, 3))
        d2[i] = r @ np.linalg.solve(S[i], r)
    return d2, S


def gate_inputs(arr, n, seed):
    """n random candidates on distinct poses of arr: a, b, z, W [n, 9] (symmetric positive definite)"""
    rng = np.random.default_rng(seed)
    N = len(arr[0])
    a = rng.integers(0, N, n).astype(np.int32); b = (a + 1 + rng.integers(0, N - 1, n)).astype(np.int32) % N
    z = rng.normal(size=(n, 3)) * [2, 2, 1]
    L = rng.normal(size=(n, 3, 3)) * 0.3 + np.eye(3) * 3
    W = np.einsum("nij,nkj->nik", L, L).reshape(n, 9)
    return a, b, z, W


def false_candidates(arr, closures, n, min_gap=50, seed=7):
    """n candidates that each take a true closure's z and W and place them on a wrong pair of poses at least min_gap apart"""
    states, fa, fb, z, W = arr
    N = len(states)
    rng = np.random.default_rng(seed)
    a, b, zz, WW = [], [], [], []
    while len(a) < n:
        f = closures[rng.integers(len(closures))]
        x, y = int(rng.integers(N)), int(rng.integers(N))
        if abs(x - y) < min_gap:
            continue
        a.append(x); b.append(y); zz.append(z[f]); WW.append(W[f])
    return np.array(a, np.int32), np.array(b, np.int32), np.array(zz, float), np.array(WW, float).reshape(-1, 9)


def held_out_closures(arr, k):
    """indices of the last k loop closures (binary factors between non-consecutive poses) and the arrays without them"""
    states, fa, fb, z, W = arr
    cl = np.nonzero((fb >= 0) & (np.abs(fa - fb) > 1))[0][-k:]
    keep = np.ones(len(fa), bool); keep[cl] = False
    return cl, (states, fa[keep], fb[keep], z[keep], W[keep])
