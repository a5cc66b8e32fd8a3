"""The numpy model of the per-factor audit (tests/support/audit_model.py) satisfies the two identities that need no tolerance of their
own, on the CPU: this pins the yardstick before any GPU number is compared with it (tests/test_gpu_factor_audit.py).

    trace identity          sum_f leverage_f + sum_i lambda_i tr(Sigma_ii) = 3 * (free nodes), because tr(Sigma A) = 3 N
    leave-one-out identity  remove f, solve the reduced system at the same lp, gate f against it: e' S^-1 e = d2_loo
"""
import numpy as np
import pytest

from tests.support import audit_model as am
from tests.support import fixed_model
from tests.support.marginal_cases import LAM, case_arrays


def _loo_picks(rows, fb):
    """three factors: the first prior, and the binary factors with the largest and the median checkability"""
    prior = int(np.nonzero(np.asarray(fb) < 0)[0][0])
    bi = np.nonzero(np.asarray(fb) >= 0)[0]
    order = bi[np.argsort(rows[bi, 3])]
    return [prior, int(order[-1]), int(order[len(order) // 2])]


def _check_identity(lp, fa, fb, z, W, f, rows, Sig, facs, fixed=()):
    """the identity itself, both sides formed in extended precision (audit_model.identity_sides: in double a lone prior's two sides lose
    the digits the identity is asked to); and the DOUBLE model's d2_loo -- audit_model.one, what the GPU tests compare with -- against it:
    to 1e-9 where the factor is checkable at all, and below the floor (the prior picks) to what double can keep there.  That bound is
    reasoned, not observed: numpy's inverse leaves Sigma with a relative error of about eps cond(A), so P W (norm at most 1: a leverage)
    and with it M = I - P W move by about eps cond(A), and M^-1 v by that over sigma_min(M); 8 covers the constants of a 3 x 3 solve"""
    if np.finfo(np.longdouble).eps > 2.0 ** -63:
        pytest.skip("numpy's longdouble is no wider than double here: the identity's two sides cannot be formed to 1e-9 for a lone prior")
    d2, loo = am.identity_sides(lp, fa, fb, z, W, LAM, f, fixed)
    assert abs(loo - d2) <= 1e-9 * abs(loo), (f, float(loo), float(d2))
    a, b, Ja, Jb, r, Wf = facs[f]
    J = Ja if Jb is None else np.hstack([Ja, Jb])
    M = np.eye(3) - J @ am.block(Sig, a, b if Jb is not None else None) @ J.T @ Wf
    free = np.setdiff1d(np.arange(len(Sig)), fixed_model.dofs(fixed)) if len(fixed) else np.arange(len(Sig))
    bound = 1e-9 if rows[f, 3] >= am.CHECK_FLOOR else max(1e-9, 8 * 2.0 ** -52 * np.linalg.cond(Sig[np.ix_(free, free)]) / np.linalg.svd(M, compute_uv=False)[-1])
    print("factor", f, "d2_loo", float(d2), "leave-one-out", float(loo), "double model", rows[f, 2], "checkability", rows[f, 3], "bound", bound)
    assert np.isfinite(rows[f, 2]) and abs(rows[f, 2] - float(d2)) <= bound * abs(float(d2)), (f, rows[f, 2], float(d2), bound)


@pytest.mark.parametrize("name", ["random0", "random1", "random2"])
def test_identities_random(name):
    states, fa, fb, z, W = case_arrays(None, name)
    rows, tol, Sig, facs = am.graph_model(states, fa, fb, z, W, LAM)
    N = len(states)
    diag = np.stack([Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(N)])
    miss = am.trace_identity(rows, diag, LAM, N)
    print(name, "trace identity miss", miss)
    assert abs(miss) <= 1e-10, miss
    assert np.all(rows[:, 1] >= -1e-12) and np.all(rows[:, 1] <= 3 + 1e-12)          # leverage in [0, rank W]
    assert np.all(rows[:, 3] >= -1e-12) and np.all(rows[:, 3] <= 1 + 1e-12)          # checkability in [0, 1]
    for f in _loo_picks(rows, fb):
        _check_identity(states, fa, fb, z, W, f, rows, Sig, facs)


@pytest.mark.parametrize("fixed", fixed_model.FIXED_SETS)
def test_identities_fixed_chain(fixed):
    sc = fixed_model.chain8()
    fa, fb, z, W = sc["plain"]
    lp = sc["start"]
    rows, tol, Sig, facs = am.graph_model(lp, fa, fb, z, W, LAM, fixed=fixed)
    N = len(lp)
    diag = np.stack([Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(N)])
    miss = am.trace_identity(rows, diag, LAM, N - len(fixed))
    assert abs(miss) <= 1e-10, miss
    for f, (a, b) in enumerate(zip(fa, fb)):          # a factor whose nodes are all fixed: P = 0
        if a in fixed and (b < 0 or b in fixed):
            assert rows[f, 1] == 0.0 and rows[f, 3] == 1.0 and rows[f, 2] == rows[f, 0], rows[f]
    for f in _loo_picks(rows, fb):
        _check_identity(lp, fa, fb, z, W, f, rows, Sig, facs, fixed)


def test_polar_form_agrees_with_the_slot_form():
    """the m-row form the model audits a polar factor in and the xyt slot the library audits (Graph-free: lib.polar_slot needs no device
    but the library; here the slot is restated) give the same four numbers: checked on a range-bearing factor with J_eff = the xyt
    Jacobians, W_eff = G' W G padded, r_eff chosen with G r_eff[:2] = r_p"""
    from tests.support import polar_model as pm
    rng = np.random.default_rng(5)
    x = np.array([[0.0, 0.0, 0.3], [1.5, 0.7, 0.0]])
    pol = (pm.RANGE_BEARING, 0, 1, np.array([1.7, 0.1]), np.array([[2500.0, 300.0], [300.0, 1e4]]))
    Ja, Jb, r, W = pm.evaluate(x, pol)
    q, Jqa, Jqb = pm.rel(x[0], x[1])
    G = pm.G(pm.RANGE_BEARING, q)
    Weff = np.zeros((3, 3)); Weff[:2, :2] = G.T @ W @ G
    reff = np.r_[np.linalg.solve(G, r), 0.0]
    Ja3 = np.vstack([Jqa, [0, 0, -1.0]]); Jb3 = np.vstack([Jqb, [0, 0, 1.0]])
    M = rng.normal(0, 1, (6, 6)); Sff = 1e-3 * (M @ M.T)
    d = rng.normal(0, 1e-2, 6)
    polar = am.one(Sff, d, (0, 1, Ja, Jb, r, W))
    slot = am.one(Sff, d, (0, 1, Ja3, Jb3, reff, Weff))
    assert np.allclose(polar, slot, rtol=1e-10, atol=0), (polar, slot)
