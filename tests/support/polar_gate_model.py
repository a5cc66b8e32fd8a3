"""numpy model of aprilsam_amd_gate_polar / aprilsam_amd_associate_polar.  TEST INFRASTRUCTURE, built on
polar_model (the true m-row factors) and gate_model (the xyt gate).

For a candidate (kind, z [m], W [m, m]), a observing b:
    q, r     position of b in a's frame and r = z - h(q), the bearing wrapped, at the states
    J_p      G [J_a J_b][:2]  (m x 6): polar_model.evaluate's Jacobians
    S  = J_p Sigma_ab J_p' + W^-1,   d2 = r' S^-1 r        Sigma_ab: the 6 x 6 joint covariance, a's unknowns first
rho^2 == 0: not available (NaN).  The association takes, per observation, the landmark of the smallest d2 (ties to the lower index) if it
passes the gate of the observation's row count, and reports the two smallest d2 whatever the gate says."""
import numpy as np

from tests.support import gate_model
from tests.support import polar_model as pm

try:
    from scipy.stats import chi2 as _chi2
    CHI2_1_999, CHI2_2_999 = float(_chi2.ppf(0.999, 1)), float(_chi2.ppf(0.999, 2))
except ImportError:          # chi^2 0.999 quantiles with 1 and 2 degrees of freedom (Abramowitz & Stegun table 26.8; 2 dof: -2 ln 0.001)
    CHI2_1_999, CHI2_2_999 = 10.827566170662733, 13.815510557964274


def jacobian(kind, pa, pb):
    """J_p [m, 6] at the states pa, pb"""
    x = np.array([pa, pb], float)
    Ja, Jb, _, _ = pm.evaluate(x, (kind, 0, 1, np.zeros(pm.rows(kind)), np.eye(pm.rows(kind))))
    return np.hstack([Ja, Jb])


def gate_one(kind, z, W, pa, pb, C):
    """(ok, d2, S [m, m])"""
    m = pm.rows(kind)
    q, _, _ = pm.rel(np.asarray(pa, float), np.asarray(pb, float))
    if q[0] * q[0] + q[1] * q[1] == 0:
        return False, np.nan, np.full((m, m), np.nan)
    r = pm.residual(kind, z, q)
    J = jacobian(kind, pa, pb)
    S = J @ np.asarray(C, float).reshape(6, 6) @ J.T + np.linalg.inv(np.asarray(W, float).reshape(m, m))
    return True, float(r @ np.linalg.solve(S, r)), S


def gate(states, a, b, cands, joint):
    """cands: list of (kind, z, W); joint [n, 6, 6] -> (ok [n], d2 [n], S: list of [m, m])"""
    out = [gate_one(k, z, W, states[i], states[j], C) for i, j, (k, z, W), C in zip(a, b, cands, joint)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), [o[2] for o in out]


def padded(S_list):
    """the library's S layout [n, 2, 2]: a 1-row S at [0, 0] with zeros behind it"""
    out = np.zeros((len(S_list), 2, 2))
    for i, S in enumerate(S_list):
        out[i, :S.shape[0], :S.shape[1]] = S
    return out


def associate(states, observer, obs, landmarks, joint, gate1=CHI2_1_999, gate2=CHI2_2_999):
    """obs: list of (kind, z, W); joint [L, 6, 6] of the pairs (observer, landmarks[l]) -> dict(best, d2_best, d2_second, d2 [m, L], unavailable)"""
    m, L = len(obs), len(landmarks)
    mat = np.full((m, L), np.nan)
    bad = 0
    for i, (k, z, W) in enumerate(obs):
        for l, b in enumerate(landmarks):
            ok, mat[i, l], _ = gate_one(k, z, W, states[observer], states[b], joint[l])
            bad += not ok
    best = np.full(m, -1, np.int32); d1 = np.full(m, np.inf); d2 = np.full(m, np.inf)
    for i, (k, _, _) in enumerate(obs):
        fin = np.nonzero(~np.isnan(mat[i]))[0]
        if len(fin) == 0:
            continue
        order = fin[np.argsort(mat[i, fin], kind="stable")]              # (stable: ties keep the lower index)
        d1[i] = mat[i, order[0]]
        if len(order) > 1:
            d2[i] = mat[i, order[1]]
        if d1[i] <= (gate2 if pm.rows(k) == 2 else gate1):
            best[i] = order[0]
    return dict(best=best, d2_best=d1, d2_second=d2, d2=mat, unavailable=bad)


def joint_blocks(Sigma, a, b):
    """[n, 6, 6] joint blocks of a dense Sigma [3N, 3N]"""
    blk = lambda i, j: Sigma[3 * i:3 * i + 3, 3 * j:3 * j + 3]
    return np.array([np.block([[blk(i, i), blk(i, j)], [blk(j, i), blk(j, j)]]) for i, j in zip(a, b)])


def dense_sigma(lp, plain, polars, lam):
    """inverse of the system a step factorises at the l_points"""
    A, _ = pm.system(np.asarray(lp, float), plain, list(polars), lam)
    return np.linalg.inv(A.toarray())


def xyt_twin(z, W, pa, pb, w_theta=1.0):
    """the xyt candidate that carries a range-bearing measurement (z [2], W [2, 2]) at the states pa, pb: z in Cartesian form with the predicted
    relative heading (a zero heading residual), W_xyt = blockdiag(G' W G, w_theta) -> (z3, W9, G)"""
    q = gate_model.predict(pa, pb)
    G = pm.G(pm.RANGE_BEARING, q[:2])
    zc = np.array([z[0] * np.cos(z[1]), z[0] * np.sin(z[1]), q[2]])
    M = G.T @ np.asarray(W, float).reshape(2, 2) @ G
    W3 = np.zeros((3, 3)); W3[:2, :2] = 0.5 * (M + M.T); W3[2, 2] = w_theta          # (mirror entries bitwise equal: gate_xyt asks for it)
    return zc, W3.reshape(9), G


# ---- the association case the CPU test pins and the GPU test reuses -----------------------------------------------------------------------
SNAKE_SEED, ASSOC_SEED = 5, 1          # picked on the CPU (tests/test_polar_gate_model.py asserts what they were picked for)


def association_case(snake_seed=None, seed=None):
    """The 6-pose snake with 8 landmarks (polar_model.snake(3, 8, n_rows=2)), solved by three Gauss-Newton steps; the newest pose observes
    every landmark within 2.5 m again: observations regenerated from the truth with the generator's noise, kinds cycling.
    -> dict(d (the snake), x (solved states), observer, landmarks [8], obs: list of (kind, z, W), truth_idx [m])"""
    snake_seed = SNAKE_SEED if snake_seed is None else snake_seed
    seed = ASSOC_SEED if seed is None else seed
    d = pm.snake(3, 8, seed=snake_seed, n_rows=2)
    x = pm.gn_steps(d["start"], d["plain"], d["polars"], 3, pm.TIKHANOV)
    n = d["n_poses"]
    observer = n - 1
    rng = np.random.default_rng(seed)
    obs, truth_idx = [], []
    kinds = (pm.RANGE_BEARING, pm.RANGE, pm.BEARING)
    for l in range(8):
        q, _, _ = pm.rel(d["truth"][observer], d["truth"][n + l])
        if np.hypot(*q) > 2.5:
            continue
        zz = pm.h(pm.RANGE_BEARING, q) + rng.normal(0, [pm.SIGMA_RHO, pm.SIGMA_BETA])
        kind = kinds[len(obs) % 3]
        if kind == pm.RANGE:
            obs.append((kind, zz[:1].copy(), np.array([[1 / pm.SIGMA_RHO ** 2]])))
        elif kind == pm.BEARING:
            obs.append((kind, zz[1:].copy(), np.array([[1 / pm.SIGMA_BETA ** 2]])))
        else:
            cr = 0.3 / (pm.SIGMA_RHO * pm.SIGMA_BETA)
            obs.append((kind, zz.copy(), np.array([[1 / pm.SIGMA_RHO ** 2, cr], [cr, 1 / pm.SIGMA_BETA ** 2]])))
        truth_idx.append(l)
    return dict(d=d, x=x, observer=observer, landmarks=np.arange(n, n + 8, dtype=np.int32), obs=obs, truth_idx=np.array(truth_idx, np.int32))
