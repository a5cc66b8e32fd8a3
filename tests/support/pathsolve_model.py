"""numpy restatement of the path solves behind aprilsam_amd_marginals_joint_any (aprilsam_amd/csrc/pathsolve.hip.h), driven by the
product's own symbolic plan.  TEST-ONLY.

The plan comes from aprilsam_amd_plan_create / plan_query (tests/support/mf_emulator.PlanView).  Each front is factorised densely
(multifrontal, as tests/support/selinv_model.SelInvModel does), then for every queried node q the three columns Y_q = L^-1 e_q are
solved along the path from q's front to the root with one dense local vector of length s + u per front, handed to the parent through
front_rel, exactly as k_path_trsm / k_path_gemm do:

    V_S = L_SS^-1 V_S,     parent[front_rel rows] = V_U - L_US V_S

and the joint block of (a, b) is [Y_a Y_b]' [Y_a Y_b] with S_ab summed over the common ancestors only (k_path_gram).
"""
import numpy as np


class PathSolveModel:
    def __init__(self, P, A):
        """P: PlanView; A: the system in node order (dense array or scipy.sparse)"""
        import scipy.sparse as sp
        self.P = P
        nF = P.nF
        perm = P.perm.astype(np.int64)
        sidx = (3 * perm[:, None] + np.arange(3)).ravel()
        Ap = sp.csc_matrix(A)[sidx][:, sidx].tocsc()
        self.idx, self.s = [], []
        for t in range(nF):
            first, nsb = int(P.front_first[t]), int(P.front_nsb[t])
            rows = P.front_rows[int(P.front_rows_ptr[t]):int(P.front_rows_ptr[t + 1])].astype(np.int64)
            blocks = np.concatenate([np.arange(first, first + nsb), rows])
            self.idx.append((3 * blocks[:, None] + np.arange(3)).ravel())
            self.s.append(3 * nsb)
        self.Lss, self.Lus = [None] * nF, [None] * nF
        upd = [None] * nF
        ch = [[] for _ in range(nF)]
        for t in range(nF):
            if P.front_parent[t] >= 0:
                ch[int(P.front_parent[t])].append(t)
        for t in range(nF):
            ix, s = self.idx[t], self.s[t]
            F = np.zeros((len(ix), len(ix)))
            F[:, :s] = Ap[ix][:, ix[:s]].toarray()
            for c in ch[t]:
                m = self.parent_map(c)
                F[np.ix_(m, m)] += upd[c]
                upd[c] = None
            Lss = np.linalg.cholesky(F[:s, :s])
            Lus = np.linalg.solve(Lss, F[s:, :s].T).T
            self.Lss[t], self.Lus[t] = Lss, Lus
            upd[t] = F[s:, s:] - Lus @ Lus.T
        self.pos = P.pos.astype(np.int64)
        self.pos_front = np.zeros(P.N, np.int64)
        for t in range(nF):
            self.pos_front[int(P.front_first[t]):int(P.front_first[t] + P.front_nsb[t])] = t
        self._cols = {}

    def parent_map(self, t):
        """scalar rows of front t's struct rows inside its parent's local vector (front_rel)"""
        P = self.P
        rel = P.front_rel[int(P.front_rows_ptr[t]):int(P.front_rows_ptr[t + 1])].astype(np.int64)
        return (3 * rel[:, None] + np.arange(3)).ravel()

    def path(self, node):
        """the fronts from the node's own front to the root"""
        t = int(self.pos_front[self.pos[node]])
        out = []
        while t >= 0:
            out.append(t)
            t = int(self.P.front_parent[t])
        return out

    def columns(self, node):
        """{front: Y_S (s x 3)} of Y = L^-1 e_node along the node's path"""
        if node in self._cols:
            return self._cols[node]
        from scipy.linalg import solve_triangular
        P = self.P
        path = self.path(node)
        t0 = path[0]
        v = np.zeros((len(self.idx[t0]), 3))
        l = 3 * (int(self.pos[node]) - int(P.front_first[t0]))
        v[l:l + 3] = np.eye(3)
        out = {}
        for t in path:
            s = self.s[t]
            ys = solve_triangular(self.Lss[t], v[:s], lower=True)
            out[t] = ys
            p = int(P.front_parent[t])
            if p < 0:
                break
            vp = np.zeros((len(self.idx[p]), 3))
            vp[self.parent_map(t)] = v[s:] - self.Lus[t] @ ys
            v = vp
        self._cols[node] = out
        return out

    def joint_any(self, a, b):
        out = np.empty((len(a), 6, 6))
        for i, (na, nb) in enumerate(zip(a, b)):
            Ya, Yb = self.columns(int(na)), self.columns(int(nb))
            Saa = sum(y.T @ y for y in Ya.values())
            Sbb = sum(y.T @ y for y in Yb.values())
            Sab = np.zeros((3, 3))
            for t in Ya:
                if t in Yb:
                    Sab += Ya[t].T @ Yb[t]
            out[i] = np.block([[Saa, Sab], [Sab.T, Sbb]])
        return out
