"""numpy model of aprilsam_amd_logdet, aprilsam_amd_logdet_sets and aprilsam_amd_info_gain_xyt (aprilsam_amd/csrc/infomeasure.hip.h, DESIGN.md
section 32), and the tolerances their tests hold the device to.  TEST-ONLY.  All values are natural logarithms.

    logdet          2 sum ln L_jj of the Cholesky factor of A restricted to the free nodes (a fixed node's block of A is the identity)
    set prefixes    ln det of the leading 3 (j + 1) x 3 (j + 1) block of the set's joint covariance, j = 0 .. k - 1
    gain prefixes   (ln det C_prefix + sum_{i <= j} ln det W_i) / 2 with C = H Sigma H' + blockdiag(W_i^-1) as joint_gate_model.joint_gate builds it

Tolerances (first order d ln det M = tr(M^-1 dM); u = 2^-53, gamma_k = k u / (1 - k u)):
    a computed Cholesky factor satisfies |dM| <= gamma_{n+1} |L| |L|' (Higham, Accuracy and Stability, Theorem 10.3), which moves ln det M
    by at most gamma_{n+1} sum_ij |M^-1|_ij (|L| |L|')_ij; the n logarithms (half an ulp each from a correctly rounded log, one ulp allowed)
    and their sum in any order add at most (n + 2) u sum_j (1 + |ln L_jj|).  The bound is TWICE the sum of the two terms: the doubling
    stands for the higher orders, as joint_gate_model.dense_tolerances does it.
"""
import numpy as np

from .inc_exact import incremental_system
from .joint_gate_model import innovation_rows, set_cov
from .selinv_model import dense_system, system_blocks

U = 2.0 ** -53


def gamma(k):
    return k * U / (1 - k * U)


def system_matrix(lp, fa, fb, z, W, lam, lam_nodes=None):
    """A = sum J' W J + diag(lambda) at lp, dense, node order"""
    Aii, Aab = system_blocks(lp, fa, fb, z, W, lam, lam_nodes)
    return dense_system(Aii, Aab, fa, fb)


def incremental_matrix(lp, fa, fb, z, W, q, n_batch, tikhanov):
    """A of the exact system of an incremental step (tests/support/inc_exact.py: incremental_system): lambda on the poses of the last batch step"""
    zz, lam = incremental_system(np.asarray(lp, float), fa, fb, z, W, q, n_batch, tikhanov)
    Aii, Aab = system_blocks(lp, fa, fb, zz, W, 0.0)
    Aii = Aii + lam[:, None, None] * np.eye(3)
    return dense_system(Aii, Aab, fa, fb)


def free_rows(N, fixed=()):
    fx = set(int(i) for i in fixed)
    return np.array([3 * i + k for i in range(N) if i not in fx for k in range(3)], int)


def free_block(A, fixed=()):
    ix = free_rows(len(A) // 3, fixed)
    return A[np.ix_(ix, ix)]


def logdet_of_factor(L, skip=(), lower=None):
    """2 sum ln L_jj; skip: columns left out, lower: a column j read one row too low (L[j + 1][j]) -- the faults the sensitivity controls plant"""
    d = np.diag(L).copy()
    if lower is not None:
        d[lower] = abs(L[lower + 1, lower])
    keep = np.ones(len(d), bool); keep[list(skip)] = False
    return 2.0 * np.log(d[keep]).sum()


def logdet(A, fixed=()):
    return logdet_of_factor(np.linalg.cholesky(free_block(A, fixed)))


def chol_logdet_bound(M):
    """the bound of the module docstring for 2 sum ln L_jj of a computed Cholesky factor of M"""
    n = len(M)
    L = np.linalg.cholesky(M)
    first = gamma(n + 1) * (np.abs(np.linalg.inv(M)) * (np.abs(L) @ np.abs(L).T)).sum()
    logs = (n + 2) * U * (1 + np.abs(np.log(np.diag(L)))).sum()
    return 2 * (first + logs)


def logdet_tolerance(A, fixed=()):
    return chol_logdet_bound(free_block(A, fixed))


def prefixes_of(M):
    """ln det of the leading 3 (j + 1) blocks of M; NaN from the first block on whose pivot is not positive"""
    n = len(M)
    out = np.full(n // 3, np.nan)
    L = np.zeros_like(M)
    acc = 0.0
    for c in range(n):
        p = M[c, c] - L[c, :c] @ L[c, :c]
        if not p > 0:
            break
        L[c, c] = np.sqrt(p)
        L[c + 1:, c] = (M[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
        acc += 2 * np.log(L[c, c])
        if c % 3 == 2:
            out[c // 3] = acc
    return out


def set_prefixes(Sig, nodes):
    return prefixes_of(set_cov(Sig, np.asarray(nodes, int)))


def set_tight_tolerance(M):
    """per prefix: the device factorises exactly the matrix the model is given (its own blocks)"""
    return np.array([chol_logdet_bound(M[:3 * j, :3 * j]) for j in range(1, len(M) // 3 + 1)])


def set_loose_tolerance(M, Sig, nodes, sig_rtol):
    """per prefix, against the dense inverse: every entry of the device's matrix within c_atol = sig_rtol x the largest entry of the nodes'
    block rows (joint_gate_model.dense_tolerances with H = I), through 2 sum_ij |M^-1|_ij"""
    c_atol = sig_rtol * max(np.abs(Sig[3 * q:3 * q + 3]).max() for q in nodes)
    return np.array([2 * c_atol * np.abs(np.linalg.inv(M[:3 * j, :3 * j])).sum() for j in range(1, len(M) // 3 + 1)])


def gain_matrix(states, a, b, W, Sig):
    """(C, H, sum-able ln det W_i) of one hypothesis; Sig: dense [3N, 3N]"""
    m = len(a)
    W = np.asarray(W, float).reshape(m, 3, 3)
    H, _ = innovation_rows(states, a, b, np.zeros((m, 3)), Sig.shape[0])
    R = np.zeros((3 * m, 3 * m))
    for i in range(m):
        R[3 * i:3 * i + 3, 3 * i:3 * i + 3] = np.linalg.inv(W[i])
    C = H @ Sig @ H.T + R
    return 0.5 * (C + C.T), H, np.array([np.linalg.slogdet(W[i])[1] for i in range(m)])


def gain_prefixes(states, a, b, W, Sig):
    C, _, lw = gain_matrix(states, a, b, W, Sig)
    return 0.5 * (prefixes_of(C) + np.cumsum(lw))


def gain_by_adding(A, H, W):
    """(slogdet(A + H' W H) - slogdet(A)) / 2: the determinant lemma by really adding the factors; W: [m, 3, 3]"""
    m = len(W)
    Wb = np.zeros((3 * m, 3 * m))
    for i in range(m):
        Wb[3 * i:3 * i + 3, 3 * i:3 * i + 3] = W[i]
    return 0.5 * (np.linalg.slogdet(A + H.T @ Wb @ H)[1] - np.linalg.slogdet(A)[1])


def _w_inverse_error(W):
    """entrywise bound of the adjugate inverse's rounding error and of ln det W's: cofactors are differences of two products (gamma_3 of the
    sum of their magnitudes), the determinant three such terms (gamma_6), one division each"""
    W = np.asarray(W, float).reshape(3, 3)
    A = np.abs(W)
    det = abs(np.linalg.det(W))
    cof = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]; c = [k for k in range(3) if k != j]
            cof[j, i] = A[r[0], c[0]] * A[r[1], c[1]] + A[r[0], c[1]] * A[r[1], c[0]]
    detabs = (A[0] * np.array([cof[0, 0], cof[1, 0], cof[2, 0]])).sum()
    rel_det = gamma(6) * detabs / det
    return gamma(4) * cof / det + np.abs(np.linalg.inv(W)) * rel_det, rel_det + U * (1 + abs(np.log(det)))


def gain_tight_tolerance(states, a, b, W, Sig):
    """per prefix, against the model on the device's OWN Sigma blocks: the factorisation and the logarithms of C as for a set, plus the
    rounding of C's entries -- |H| |dSigma| |H|' with dSigma = gamma_16 |Sigma| (two 6-term products and the sum of four blocks per
    entry), the adjugate inverse of W_i on the diagonal -- through sum_ij |C^-1|_ij, plus the error of sum ln det W_i; halved like the gain"""
    m = len(a)
    Wm = np.asarray(W, float).reshape(m, 3, 3)
    C, H, lw = gain_matrix(states, a, b, W, Sig)
    dC = np.abs(H) @ (gamma(16) * np.abs(Sig)) @ np.abs(H).T
    dlw = np.zeros(m)
    for i in range(m):
        dWi, dlw[i] = _w_inverse_error(Wm[i])
        dC[3 * i:3 * i + 3, 3 * i:3 * i + 3] += dWi + U * np.abs(C[3 * i:3 * i + 3, 3 * i:3 * i + 3])
    out = np.empty(m)
    for j in range(1, m + 1):
        n = 3 * j
        out[j - 1] = 0.5 * (chol_logdet_bound(C[:n, :n]) + 2 * (np.abs(np.linalg.inv(C[:n, :n])) * dC[:n, :n]).sum() + 2 * dlw[:j].sum() + (j + 2) * U * np.abs(lw[:j]).sum())
    return out


def gain_loose_tolerance(states, a, b, W, Sig, sig_rtol):
    """per prefix, against the dense inverse: c_atol of joint_gate_model.dense_tolerances times 2 sum_ij |C^-1|_ij, halved like the gain"""
    from .joint_gate_model import dense_tolerances
    m = len(a)
    C, _, _ = gain_matrix(states, a, b, W, Sig)
    _, c_atol = dense_tolerances(states, a, b, np.zeros((m, 3)), C, Sig, sig_rtol)
    return np.array([0.5 * 2 * c_atol * np.abs(np.linalg.inv(C[:3 * j, :3 * j])).sum() for j in range(1, m + 1)])
