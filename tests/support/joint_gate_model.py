"""numpy model of aprilsam_amd_marginals_set and aprilsam_amd_gate_xyt_joint (k_block_chol<JointGate>, aprilsam_amd/csrc/jointgate.hip.h).  TEST-ONLY.

For a hypothesis of m candidate xyt measurements (a_i, b_i, z_i, W_i), with Sigma the dense inverse of the factorised system
(tests/support/selinv_model.py: system_blocks, dense_system):
    r_i, J_ai, J_bi    as tests/support/gate_model.py: jacobians
    H                  3m x 3N, J_ai and J_bi in the columns of a_i and b_i
    C  = H Sigma H' + blockdiag(W_i^-1)
    C  = L L', y = L^-1 r;  prefix j = sum of y_t^2 over t < 3 (j + 1): the joint distance of the first j + 1 candidates
"""
import numpy as np

from .gate_model import jacobians
from .selinv_model import dense_system, system_blocks


def dense_sigma(lp, fa, fb, z, W, lam, lam_nodes=None, fixed=()):
    """inv(A) of the system linearised at lp; the rows and columns of the `fixed` nodes zero (they are constants: the free nodes'
    covariance is the inverse of the free block)"""
    Aii, Aab = system_blocks(lp, fa, fb, z, W, lam, lam_nodes)
    A = dense_system(Aii, Aab, fa, fb)
    N = len(lp)
    free = np.array([3 * i + k for i in range(N) if i not in set(fixed) for k in range(3)], int)
    Sig = np.zeros_like(A)
    Sig[np.ix_(free, free)] = np.linalg.inv(A[np.ix_(free, free)])
    return 0.5 * (Sig + Sig.T)


def set_cov(Sig, nodes):
    """the (3k) x (3k) joint covariance of the listed nodes (a node may repeat)"""
    ix = np.concatenate([np.r_[3 * q:3 * q + 3] for q in nodes]) if len(nodes) else np.zeros(0, int)
    return Sig[np.ix_(ix, ix)]


def innovation_rows(states, a, b, z, n_unknowns):
    """H [3m, n_unknowns] and the stacked residual r [3m] of the candidates at the states"""
    states = np.asarray(states, float)
    m = len(a)
    z = np.asarray(z, float).reshape(m, 3)
    H = np.zeros((3 * m, n_unknowns)); r = np.empty(3 * m)
    for i in range(m):
        Ja, Jb, ri = jacobians(states[a[i]], states[b[i]], z[i])
        H[3 * i:3 * i + 3, 3 * a[i]:3 * a[i] + 3] += Ja
        H[3 * i:3 * i + 3, 3 * b[i]:3 * b[i] + 3] += Jb
        r[3 * i:3 * i + 3] = ri
    return H, r


def joint_gate(states, a, b, z, W, Sig):
    """(prefix [m], C [3m, 3m], r [3m]) of one hypothesis; Sig: dense [3N, 3N]"""
    m = len(a)
    W = np.asarray(W, float).reshape(m, 3, 3)
    H, r = innovation_rows(states, a, b, z, Sig.shape[0])
    R = np.zeros((3 * m, 3 * m))
    for i in range(m):
        R[3 * i:3 * i + 3, 3 * i:3 * i + 3] = np.linalg.inv(W[i])
    C = H @ Sig @ H.T + R
    C = 0.5 * (C + C.T)
    y = np.linalg.solve(np.linalg.cholesky(C), r)
    return np.cumsum(y * y)[2::3], C, r


def dense_tolerances(states, a, b, z, C, Sig, sig_rtol):
    """(rtol of the prefixes, atol of C) for a device result compared with the model on the DENSE inverse, when the device's Sigma blocks
    agree with that inverse to sig_rtol of their block rows' largest entry (tests/support/sigma_compare.py): |dC| <= |H| |dSigma| |H|'
    entrywise, and a Mahalanobis distance moves by at most cond(C) |dC| / |C| (2-norms; first order), doubled for the higher orders"""
    H, _ = innovation_rows(states, a, b, z, Sig.shape[0])
    nodes = np.unique(np.r_[a, b])
    scale = max(np.abs(Sig[3 * q:3 * q + 3]).max() for q in nodes)
    c_atol = np.abs(H).sum(axis=1).max() ** 2 * sig_rtol * scale
    ev = np.linalg.eigvalsh(C)
    return 2 * (3 * len(a)) * c_atol / ev[0], c_atol
