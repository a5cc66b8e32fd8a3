"""numpy restatement of the whole-tree solves behind aprilsam_amd_solve / aprilsam_amd_marginals_cross /
aprilsam_amd_relative_covariances (aprilsam_amd/csrc/treesolve.hip.h), driven by the product's own symbolic plan.  TEST-ONLY.

The plan comes from aprilsam_amd_plan_create / plan_query (tests/support/mf_emulator.PlanView); the per-front L_SS and L_US are those
of tests/support/pathsolve_model.PathSolveModel.  Every front holds a dense local block of (s + u) x ncol, own rows first:

    forward, leaves to root    own rows = B at node -> pos -> local row; all rows += the children's V_U through front_rel, child by
                               child in ascending front id (a parent-side sum);  V_S = L_SS^-1 V_S;  V_U = V_U - L_US V_S
    backward, root to leaves   V_U = the parent's rows at front_rel;  V_S = V_S - L_US' V_U;  V_S = L_SS^-T V_S

and X is read from the own rows in node order.  A mismatch between the plan's maps and what the kernels assume shows up here, without
a GPU.
"""
import numpy as np
from scipy.linalg import solve_triangular

from .gate_model import jacobians
from .pathsolve_model import PathSolveModel

FULL, FORWARD, BACKWARD = 0, 1, 2


class TreeSolveModel:
    def __init__(self, P, A):
        """P: PlanView; A: the system in node order (dense array or scipy.sparse)"""
        self.P = P
        self.M = PathSolveModel(P, A)
        nF = P.nF
        self.children = [[] for _ in range(nF)]
        for t in range(nF):                                  # (ascending t: every list in ascending front id)
            p = int(P.front_parent[t])
            if p >= 0:
                assert p > t
                self.children[p].append(t)
        depth = np.zeros(nF, int)
        for t in range(nF - 1, -1, -1):
            p = int(P.front_parent[t])
            depth[t] = 0 if p < 0 else depth[p] + 1
        self.levels = [np.nonzero(depth == d)[0] for d in range(int(depth.max()) + 1 if nF else 0)]      # root first
        perm = P.perm.astype(np.int64)
        # own scalar rows of front t in node coordinates: node of position first + k
        self.own = []
        for t in range(nF):
            first, nsb = int(P.front_first[t]), int(P.front_nsb[t])
            nodes = perm[first:first + nsb]
            self.own.append((3 * nodes[:, None] + np.arange(3)).ravel())

    def solve(self, B, mode=FULL):
        """B: [3N, ncol] in node order; returns X of the same shape"""
        M, P = self.M, self.P
        B = np.asarray(B, float)
        nF = P.nF
        V = [None] * nF
        if mode != BACKWARD:
            for lev in reversed(self.levels):
                for t in lev:
                    s = M.s[t]
                    v = np.zeros((len(M.idx[t]), B.shape[1]))
                    v[:s] = B[self.own[t]]
                    for c in self.children[t]:               # parent-side sum, ascending child id
                        np.add.at(v, M.parent_map(c), V[c][M.s[c]:])
                    v[:s] = solve_triangular(M.Lss[t], v[:s], lower=True)
                    v[s:] -= M.Lus[t] @ v[:s]
                    V[t] = v
        else:
            for t in range(nF):
                V[t] = np.zeros((len(M.idx[t]), B.shape[1]))
                V[t][:M.s[t]] = B[self.own[t]]
        if mode != FORWARD:
            for lev in self.levels:
                for t in lev:
                    s = M.s[t]
                    v = V[t]
                    p = int(P.front_parent[t])
                    if p >= 0:
                        v[s:] = V[p][M.parent_map(t)]
                    v[:s] -= M.Lus[t].T @ v[s:]
                    v[:s] = solve_triangular(M.Lss[t], v[:s], lower=True, trans="T")
        X = np.empty_like(B)
        for t in range(nF):
            X[self.own[t]] = V[t][:M.s[t]]
        return X

    def cross(self, anchor, nodes=None):
        """[n, 3, 3] Sigma_{node, anchor}, the node's unknowns as rows"""
        N = self.P.N
        E = np.zeros((3 * N, 3))
        E[3 * anchor:3 * anchor + 3] = np.eye(3)
        X = self.solve(E, FULL)
        nodes = np.arange(N) if nodes is None else np.asarray(nodes)
        return X.reshape(N, 3, 3)[nodes]


def relative_covariances(states, anchor, nodes, Saa, Sii, Sia):
    """[n, 3, 3]: [J_a J_i] [[S_aa S_ai]; [S_ia S_ii]] [J_a J_i]' with the xyt Jacobians at `states`; zeros for i == anchor.
    Saa: [3, 3]; Sii, Sia: [n, 3, 3] (Sia: the node's unknowns as rows)."""
    states = np.asarray(states, float)
    out = np.zeros((len(nodes), 3, 3))
    for k, i in enumerate(nodes):
        if i == anchor:
            continue
        Ja, Ji, _ = jacobians(states[anchor], states[i], np.zeros(3))
        J = np.hstack([Ja, Ji])
        C = np.block([[Saa, Sia[k].T], [Sia[k], Sii[k]]])
        out[k] = J @ C @ J.T
    return out


def backward_error(A, X, B):
    """per column: max_i |A X - B|_i / (|A| |X| + |B|)_i  (A: scipy.sparse or dense; X, B: [3N, ncol])"""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    num = np.abs(A @ X - B)
    den = abs(A) @ np.abs(X) + np.abs(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(den > 0, num / den, 0.0)
    return q.max(axis=0)


# The backward-error limits of tests/test_gpu_treesolve.py.  1e-12 everywhere (scipy's splu reaches 1.6e-15 on M3500 and the random
# graphs), except where 100 x the backward error splu itself reaches on that graph and right-hand side is larger: then that figure
# (tests/test_treesolve_model.py computes and prints splu's; measured values in its header).
OMEGA_LIMIT = 1e-12
LATTICE_OMEGA_LIMIT = {60: 1.5e-12, 316: 1.9e-12}      # splu: 1.499e-14 (K = 60, 17 columns), 1.896e-14 (K = 316, 3 columns)


def rhs_columns(N, nrhs, seed):
    """[3N, nrhs] right-hand sides: column 0 seeded normal, 1 the x unit column of the middle pose, 2 zero, 3 and 4 the middle pose's y and
    theta unit columns, the rest seeded normal"""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(3 * N, nrhs))
    mid = N // 2
    for col, k in ((1, 0), (3, 1), (4, 2)):
        if col < nrhs:
            B[:, col] = 0.0
            B[3 * mid + k, col] = 1.0
    if nrhs > 2:
        B[:, 2] = 0.0
    return B
