"""The numpy model of range / bearing / range-bearing factors (tests/support/polar_model.py) against itself: its
Jacobians against central differences, its normal equations against a dense assembly from those Jacobians, its Gauss-Newton and LM runs on
the generated snake graphs (they reach the noise floor from a dead-reckoned start), and the generator's own promises.  No GPU, no
library."""
import numpy as np
import pytest

from tests.support import lm_model
from tests.support import polar_model as pm
from tests.support.normal_eq import mod2pi

KINDS = (pm.RANGE, pm.BEARING, pm.RANGE_BEARING)


def _random_polar(rng, kind, a=0, b=1):
    m = pm.rows(kind)
    M = rng.normal(size=(m, m))
    W = M @ M.T + np.diag(rng.uniform(1, 50, m))
    z = np.array([rng.uniform(0.1, 6.0), rng.uniform(-np.pi, np.pi)])
    return (kind, a, b, (z[:1] if kind == pm.RANGE else z[1:] if kind == pm.BEARING else z).copy(), 0.5 * (W + W.T))


@pytest.mark.parametrize("kind", KINDS)
def test_jacobians_against_central_differences(kind):
    rng = np.random.default_rng(kind)
    worst = 0.0
    for _ in range(200):
        x = rng.normal(0, 3, (2, 3))
        pol = _random_polar(rng, kind)
        Ja, Jb, r, _ = pm.evaluate(x, pol)
        rho = np.hypot(*pm.rel(x[0], x[1])[0])
        eps = 1e-6 * min(1.0, rho)
        for n, J in ((0, Ja), (1, Jb)):
            for k in range(3):
                xp, xm = x.copy(), x.copy()
                xp[n, k] += eps; xm[n, k] -= eps
                d = pm.evaluate(xp, pol)[2] - pm.evaluate(xm, pol)[2]
                if kind != pm.RANGE:
                    d[-1] = mod2pi(d[-1])
                fd = -d / (2 * eps)                                  # r = z - h: dh/dx = -dr/dx
                scale = max(1.0, np.abs(J).max())
                worst = max(worst, np.abs(fd - J[:, k]).max() / scale)
    # central differences with a step of 1e-6 rho on a function with third derivatives of order 1 / rho^3: 1e-12 / rho^2 relative to
    # a Jacobian of order 1 / rho, plus round-off 1e-16 / 1e-6
    assert worst < 1e-7, worst
    assert np.all(Jb[:, 2] == 0)                                     # b's heading never enters


def test_bearing_residual_wraps():
    x = np.array([[0.0, 0.0, 0.0], [-1.0, 1e-3, 0.3]])                # beta just below +pi
    r = pm.residual(pm.BEARING, [-np.pi + 1e-3], pm.rel(x[0], x[1])[0])
    assert abs(r[0] - (1e-3 + (np.pi - np.arctan2(1e-3, -1.0)))) < 1e-12      # (not 2 pi away)


def test_zero_range_is_silent():
    x = np.array([[1.0, 2.0, 0.4], [1.0, 2.0, -1.0]])
    for kind in KINDS:
        Ja, Jb, r, W = pm.evaluate(x, _random_polar(np.random.default_rng(5), kind))
        assert np.all(Ja == 0) and np.all(Jb == 0) and np.all(np.isfinite(r))


def test_system_is_the_dense_sum():
    d = pm.snake(4, 3, seed=3)
    x = d["start"]
    A, B = pm.system(x, d["plain"], d["polars"], 1e-4)
    A0, B0 = lm_model.system(x, *d["plain"], 1e-4)
    Ad, Bd = A0.toarray(), B0.copy()
    for pol in d["polars"]:
        Ja, Jb, r, W = pm.evaluate(x, pol)
        J = np.zeros((len(r), Ad.shape[0]))
        J[:, 3 * pol[1]:3 * pol[1] + 3] = Ja; J[:, 3 * pol[2]:3 * pol[2] + 3] = Jb
        Ad += J.T @ W @ J; Bd += J.T @ W @ r
    assert np.abs(A.toarray() - Ad).max() <= 1e-12 * np.abs(Ad).max()
    assert np.abs(B - Bd).max() <= 1e-12 * np.abs(Bd).max()
    assert np.abs(A.toarray() - A.toarray().T).max() <= 1e-12 * np.abs(Ad).max()


@pytest.mark.parametrize("K,L", [(4, 3), (6, 8)])
def test_generator(K, L):
    d = pm.snake(K, L, seed=1)
    n = d["n_poses"]
    assert n == K * K and len(d["truth"]) == n + L == len(d["start"])
    kinds = {p[0] for p in d["polars"]}
    assert kinds == set(KINDS)
    assert all(p[1] < n <= p[2] for p in d["polars"])                   # poses observe landmarks
    # every node and factor arrives exactly once, and a factor never before its nodes
    have, nf, npol = set(), 0, 0
    for ev in d["events"]:
        for what, i in ev:
            if what == "node":
                assert i not in have; have.add(i)
            elif what == "plain":
                assert i == nf and d["plain"][0][i] in have and (d["plain"][1][i] < 0 or d["plain"][1][i] in have); nf += 1
            else:
                assert i == npol and d["polars"][i][1] in have and d["polars"][i][2] in have; npol += 1
    assert have == set(range(n + L)) and nf == len(d["plain"][0]) and npol == len(d["polars"])
    # the measurements are the truth's up to the stated noise: chi2 of the truth is of the order of the residual count
    dof = 3 * len(d["plain"][0]) + sum(pm.rows(p[0]) for p in d["polars"])
    assert pm.cost(d["truth"], d["plain"], d["polars"]) < 3.0 * dof


def test_gauss_newton_and_lm_reach_the_noise_floor():
    d = pm.snake(6, 8, seed=2)
    plain, polars = d["plain"], d["polars"]
    F0 = pm.cost(d["start"], plain, polars)
    x = pm.gn_steps(d["start"], plain, polars, 6, pm.TIKHANOV)
    dof = 3 * len(plain[0]) + sum(pm.rows(p[0]) for p in polars)
    assert pm.cost(x, plain, polars) < min(F0, 2.0 * dof)
    r = pm.optimize(d["start"], plain, polars, max_iters=30)
    assert r["status"] in (lm_model.CONVERGED_F, lm_model.CONVERGED_X) and r["accepted"] >= 2
    assert r["F_final"] <= pm.cost(x, plain, polars) * (1 + 1e-6)
    # the accepted steps decrease F, and the model decrease is positive on every one of them
    acc = r["trace"][:, 3] == 1
    assert np.all(np.diff(np.concatenate([[r["F_initial"]], r["trace"][acc, 0]])) < 0)
    # poses within 5 sigma of the odometry noise accumulated over the path, landmarks within 0.2 m
    n = d["n_poses"]
    assert np.abs(r["x"][:n, :2] - d["truth"][:n, :2]).max() < 0.5
    assert np.abs(r["x"][n:, :2] - d["truth"][n:, :2]).max() < 0.5


def test_pred_is_the_quadratic_models_decrease():
    d = pm.snake(4, 3, seed=4)
    x, plain, polars = d["start"], d["plain"], d["polars"]
    A, B = pm.system(x, plain, polars, 0.0)
    h = np.random.default_rng(0).normal(0, 1e-2, 3 * len(x))
    want = 2 * h @ B - h @ (A @ h)                                  # F(x) - |r - J h|_W^2
    got = pm.pred(x, h, plain, polars)
    assert abs(got - want) <= 1e-10 * max(abs(want), 1.0)


def test_gnc_with_xyt_candidates_beside_polar_factors():
    """the GNC schedule of tests/support/gnc_model.py on a snake with false xyt closures (the candidates) and landmarks observed by
    range-bearing factors (never candidates): the false closures end with weight 0, the true ones with weight 1"""
    from tests.support import gnc_model as gm
    sc = gm.snake(6, 3, 1)
    truth, start, polars = pm.with_landmarks(sc["truth"], sc["start"], 6, seed=1)
    r = pm.gnc_optimize(start, sc["plain"], polars, sc["cand"], gm.TLS)
    assert r["status"] == gm.FINISHED
    false = np.asarray(sc["is_false"], bool)
    assert np.all(r["weights"][false] == 0.0) and np.all(r["weights"][~false] == 1.0)
    n = len(sc["truth"])
    assert gm.position_error(r["x"][:n], sc["truth"]) < 0.15
    assert np.abs(r["x"][n:, :2] - truth[n:, :2]).max() < 0.15
