"""Matrix-free check of marginal covariances: for every pose i,  sum_{j in N(i) + {i}} A_ij Sigma_ji = I_3.

TEST-ONLY.  Every A_ij != 0 (i != j) comes from a factor joining i and j, and the pattern of A lies inside the pattern of L, so
the diagonal blocks Sigma_ii and the joint blocks of the factors' end poses -- exactly what aprilsam_amd_marginals /
aprilsam_amd_marginals_joint return -- are all the identity needs.  Cost O(N + F): usable on the 10^6-pose lattice, where
nothing can invert A.  The residual of pose i is reported relative to the size of the terms it sums, max over the 3 x 3 block
of  sum_j |A_ij| |Sigma_ji|  (elementwise products of absolute values): a correct Sigma leaves it at rounding, a wrong block at
order one."""
import numpy as np


def identity_residual(Aii, Aab, fa, fb, diag, joint):
    """Aii [N,3,3], Aab [F,3,3] (tests/support/selinv_model.system_blocks); diag [N,3,3] Sigma_ii; joint [F,6,6] joint blocks of
    (fa[f], fb[f]) (rows of priors are ignored).  -> dict(rel_max, rel_per_pose [N], max_abs)"""
    fa = np.asarray(fa); fb = np.asarray(fb)
    N = len(Aii)
    R = np.einsum("nij,njk->nik", Aii, diag) - np.eye(3)
    S = np.einsum("nij,njk->nik", np.abs(Aii), np.abs(diag))
    bi = np.nonzero(fb >= 0)[0]
    if len(bi):
        A_ab = Aab[bi]
        J = joint[bi]
        S_ba = J[:, 3:, :3]              # Sigma_{b a}
        S_ab = J[:, :3, 3:]
        np.add.at(R, fa[bi], np.einsum("fij,fjk->fik", A_ab, S_ba))
        np.add.at(S, fa[bi], np.einsum("fij,fjk->fik", np.abs(A_ab), np.abs(S_ba)))
        A_ba = np.transpose(A_ab, (0, 2, 1))
        np.add.at(R, fb[bi], np.einsum("fij,fjk->fik", A_ba, S_ab))
        np.add.at(S, fb[bi], np.einsum("fij,fjk->fik", np.abs(A_ba), np.abs(S_ab)))
    per = np.abs(R).reshape(N, 9).max(axis=1) / np.maximum(S.reshape(N, 9).max(axis=1), 1e-300)
    return dict(rel_max=float(per.max()) if N else 0.0, rel_per_pose=per, max_abs=float(np.abs(R).max()) if N else 0.0)
