"""numpy restatement of the selected inversion (aprilsam_amd/csrc/selinv.hip.h) driven by the product's own symbolic plan.

TEST-ONLY.  The plan comes from aprilsam_amd_plan_create / plan_query (tests/support/mf_emulator.PlanView): front rows, the
child -> parent block maps (front_rel), own blocks, parents, levels, the elimination order.  Each front is factorised densely
(multifrontal: its own columns of A plus the children's update blocks, extend-added through front_rel), then Sigma = A^-1 is
recovered root to leaves with the recurrences the kernels use:

    Sig_UU  gathered from the parent's Sig_FF through front_rel (read the other way)
    Sig_US = -Sig_UU L_US L_SS^-1
    Sig_SS = L_SS^-T (L_SS^-1 - L_US^T Sig_US)

and the blocks a caller asks for are read as k_marginal_extract reads them (the front owning the earlier-eliminated pose,
a row lookup for the other).  A mismatch between the plan and what the kernels assume shows up here, without a GPU.
"""
import numpy as np

from .normal_eq import linearise


def system_blocks(lp, fa, fb, z, W, lam, lam_nodes=None):
    """per-node diagonal blocks Aii [N,3,3] (lambda included) and per-factor cross blocks Aab [F,3,3] = J_a' W J_b (zero for priors)
    of A = sum_f J_f' W_f J_f + diag(lambda) at lp.  lam_nodes: nodes [0, lam_nodes) carry lambda (default: all)."""
    lp = np.asarray(lp, float).reshape(-1, 3)
    fa = np.asarray(fa); fb = np.asarray(fb)
    W = np.asarray(W, float).reshape(-1, 3, 3)
    N = len(lp)
    Ja, Jb, _ = linearise(lp, fa, fb, z)
    JaW = np.einsum("fki,fkl->fil", Ja, W)
    JbW = np.einsum("fki,fkl->fil", Jb, W)
    Aii = np.zeros((N, 3, 3))
    np.add.at(Aii, fa, np.einsum("fil,flj->fij", JaW, Ja))
    binary = fb >= 0
    np.add.at(Aii, fb[binary], np.einsum("fil,flj->fij", JbW[binary], Jb[binary]))
    n_lam = N if lam_nodes is None else int(lam_nodes)
    Aii[:n_lam] += lam * np.eye(3)
    Aab = np.einsum("fil,flj->fij", JaW, Jb)
    return Aii, Aab


def dense_system(Aii, Aab, fa, fb):
    """A as a dense [3N, 3N] matrix in node order"""
    N = len(Aii)
    A = np.zeros((3 * N, 3 * N))
    for i in range(N):
        A[3 * i:3 * i + 3, 3 * i:3 * i + 3] += Aii[i]
    for f in range(len(fa)):
        a, b = int(fa[f]), int(fb[f])
        if b < 0:
            continue
        A[3 * a:3 * a + 3, 3 * b:3 * b + 3] += Aab[f]
        A[3 * b:3 * b + 3, 3 * a:3 * a + 3] += Aab[f].T
    return A


def sparse_system(Aii, Aab, fa, fb):
    """the same as a scipy.sparse CSC matrix"""
    import scipy.sparse as sp
    N = len(Aii)
    fa = np.asarray(fa); fb = np.asarray(fb)
    rows, cols, vals = [], [], []
    ii, jj = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    n3 = 3 * np.arange(N)
    rows.append((n3[:, None, None] + ii).ravel()); cols.append((n3[:, None, None] + jj).ravel()); vals.append(Aii.ravel())
    bi = np.nonzero(fb >= 0)[0]
    a3, b3 = 3 * fa[bi], 3 * fb[bi]
    rows.append((a3[:, None, None] + ii).ravel()); cols.append((b3[:, None, None] + jj).ravel()); vals.append(Aab[bi].ravel())
    rows.append((b3[:, None, None] + jj).ravel()); cols.append((a3[:, None, None] + ii).ravel()); vals.append(Aab[bi].ravel())
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * N, 3 * N))


class SelInvModel:
    """Sigma on the pattern of the plan's factor; .marginals(nodes) / .joint(a, b) as the C entry points return them"""

    def __init__(self, P, A):
        """P: PlanView; A: the system in node order (dense array or scipy.sparse)"""
        import scipy.sparse as sp
        self.P = P
        nF = P.nF
        perm = P.perm.astype(np.int64)
        sidx = (3 * perm[:, None] + np.arange(3)).ravel()           # scalar index of position-ordered unknowns
        Ap = sp.csc_matrix(A)[sidx][:, sidx].tocsc()
        self.idx = []                                               # per front: scalar position indices, own first then struct rows
        self.s = []
        for t in range(nF):
            first, nsb = int(P.front_first[t]), int(P.front_nsb[t])
            rows = P.front_rows[int(P.front_rows_ptr[t]):int(P.front_rows_ptr[t + 1])].astype(np.int64)
            blocks = np.concatenate([np.arange(first, first + nsb), rows])
            self.idx.append((3 * blocks[:, None] + np.arange(3)).ravel())
            self.s.append(3 * nsb)
        # multifrontal factorisation, children before parents (post order)
        self.Lss, self.Lus = [None] * nF, [None] * nF
        upd = [None] * nF
        ch = [[] for _ in range(nF)]
        for t in range(nF):
            if P.front_parent[t] >= 0:
                ch[int(P.front_parent[t])].append(t)
        for t in range(nF):
            ix, s = self.idx[t], self.s[t]
            C = len(ix)
            F = np.zeros((C, C))
            F[:, :s] = Ap[ix][:, ix[:s]].toarray()
            for c in ch[t]:
                m = self.parent_map(c)
                F[np.ix_(m, m)] += upd[c]
                upd[c] = None
            Lss = np.linalg.cholesky(F[:s, :s])
            Lus = np.linalg.solve(Lss, F[s:, :s].T).T
            self.Lss[t], self.Lus[t] = Lss, Lus
            upd[t] = F[s:, s:] - Lus @ Lus.T
        # selected inversion, parents before children
        self.sig = [None] * nF
        for t in range(nF - 1, -1, -1):
            s = self.s[t]
            u = len(self.idx[t]) - s
            Linv = np.linalg.inv(self.Lss[t])
            Sig = np.zeros((s + u, s + u))
            if u:
                p = int(P.front_parent[t])
                m = self.parent_map(t)
                Suu = self.sig[p][np.ix_(m, m)]
                X = self.Lus[t] @ Linv
                Sus = -Suu @ X
                Sig[s:, s:] = Suu
                Sig[s:, :s] = Sus
                Sig[:s, s:] = Sus.T
                Sig[:s, :s] = Linv.T @ Linv - X.T @ Sus
            else:
                Sig[:s, :s] = Linv.T @ Linv
            self.sig[t] = Sig
        self.pos = P.pos.astype(np.int64)
        self.pos_front = np.zeros(P.N, np.int64)
        for t in range(nF):
            self.pos_front[int(P.front_first[t]):int(P.front_first[t] + P.front_nsb[t])] = t

    def parent_map(self, t):
        """scalar rows of front t's struct rows inside its parent's Sig_FF (front_rel, as k_selinv_gather reads it)"""
        P = self.P
        rel = P.front_rel[int(P.front_rows_ptr[t]):int(P.front_rows_ptr[t + 1])].astype(np.int64)
        return (3 * rel[:, None] + np.arange(3)).ravel()

    def _local(self, t, q):
        P = self.P
        first, nsb = int(P.front_first[t]), int(P.front_nsb[t])
        if first <= q < first + nsb:
            return 3 * (q - first)
        rows = P.front_rows[int(P.front_rows_ptr[t]):int(P.front_rows_ptr[t + 1])]
        k = int(np.searchsorted(rows, q))
        return 3 * nsb + 3 * k if k < len(rows) and rows[k] == q else -1

    def marginals(self, nodes=None):
        nodes = np.arange(self.P.N) if nodes is None else np.asarray(nodes)
        out = np.empty((len(nodes), 3, 3))
        for i, n in enumerate(nodes):
            q = self.pos[n]; t = self.pos_front[q]; l = self._local(t, q)
            out[i] = self.sig[t][l:l + 3, l:l + 3]
        return out

    def joint(self, a, b):
        """as k_marginal_extract: from the front owning the earlier-eliminated pose; one decision per pair -- both poses among that
        front's rows, or all 36 values NaN"""
        out = np.full((len(a), 6, 6), np.nan)
        for i, (na, nb) in enumerate(zip(a, b)):
            pa, pb = self.pos[na], self.pos[nb]
            t = self.pos_front[min(pa, pb)]
            la, lb = self._local(t, pa), self._local(t, pb)
            if la < 0 or lb < 0:
                continue
            ix = np.r_[la:la + 3, lb:lb + 3]
            out[i] = self.sig[t][np.ix_(ix, ix)]
        return out
