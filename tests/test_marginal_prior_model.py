"""The numpy model of DESIGN.md section 24 (tests/support/marginal_prior_model.py) pinned on itself: eliminating M densely from the full
system gives the same dx on the kept nodes as solving the reduced system with the prior, for a regular and a rank-deficient Lambda; the
square-root form reproduces Lambda, eta and the chi^2 term; the heading wrap; float64 against longdouble.  No GPU, no library."""
import numpy as np
import pytest

from tests.support import marginal_prior_model as mm
from tests.support.gaussian_graphs import snake


def chain(n, seed, closures=()):
    sc = snake(n, seed, closures)
    return sc["start"], sc["fa"], sc["fb"], sc["z"], sc["W"]


@pytest.mark.parametrize("remove,rank", [([0], 3), ([7], None), ([3], 3), ([2, 3], 6), ([1, 4, 6], None)])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_reduced_system_with_the_prior_gives_the_full_system_s_step(remove, rank, dtype):
    lp, fa, fb, z, W = chain(8, 5, closures=[(1, 5), (2, 6)])
    N = len(lp)
    H, g = mm.dense_system(lp, fa, fb, z, W, dtype)
    dx_full = mm.solve_spd(H, g, dtype).reshape(N, 3)
    keep, xbar, eta, Lam = mm.marginal_prior(lp, fa, fb, z, W, remove, dtype)
    FM, B = mm.blanket(fa, fb, remove)
    assert list(keep) == B and np.array_equal(xbar, lp[B]) and np.array_equal(Lam, Lam.T)
    rest = [f for f in range(len(fa)) if f not in FM]
    Hr, gr = mm.dense_system(lp, fa, fb, z, W, dtype, only=rest)
    mm.gaussian_system(Hr, gr, lp, keep, xbar, eta, Lam)          # (delta = 0: the prior's g is eta)
    kept = [i for i in range(N) if i not in remove]
    rows = mm._rows(kept)
    dx_red = mm.solve_spd(Hr[np.ix_(rows, rows)], gr[rows], dtype).reshape(-1, 3)
    tol = 1e-9 if dtype is np.float64 else 1e-12
    assert float(np.max(np.abs(dx_red - dx_full[kept]))) < tol
    if rank is not None:          # a blanket the removed nodes tie to nothing absolute: a pure relative constraint
        _, r, _, _ = mm.pivoted_cholesky(Lam.astype(np.float64))
        want = 3 * len(B) if 0 in remove else rank        # (the prior on node 0 goes into the marginal when node 0 is removed: regular)
        assert r == want, (r, want)


def test_float64_and_longdouble_agree_to_rounding():
    lp, fa, fb, z, W = chain(9, 6, closures=[(0, 4), (3, 8)])
    a = mm.marginal_prior(lp, fa, fb, z, W, [4, 5])
    b = mm.marginal_prior(lp, fa, fb, z, W, [4, 5], np.longdouble)
    assert np.array_equal(a[0], b[0])
    scale = float(np.max(np.abs(b[3])))
    assert 0 < float(np.max(np.abs(a[3] - b[3]))) < 1e-10 * scale and float(np.max(np.abs(a[2] - b[2]))) < 1e-10 * scale


@pytest.mark.parametrize("case", ["regular", "rank3of6", "zero"])
def test_square_root_form(case):
    rng = np.random.default_rng(7)
    if case == "regular":
        Q = rng.normal(size=(6, 6)); Lam = Q @ Q.T + np.eye(6); want = 6
    elif case == "rank3of6":      # J'WJ of one relative constraint between two poses
        J = np.hstack([-np.eye(3) + 0.1 * rng.normal(size=(3, 3)), np.eye(3)]); Lam = J.T @ np.diag([30.0, 20.0, 100.0]) @ J; want = 3
    else:
        Lam = np.zeros((6, 6)); want = 0
    Lam = 0.5 * (Lam + Lam.T)
    eta = Lam @ rng.normal(size=6)                                # in the range of Lambda
    for dtype in (np.float64, np.longdouble):
        R, d, c0 = mm.sqrt_form(eta, Lam, dtype)
        assert R.shape == (want, 6)
        tol = 1e-12 * max(1.0, float(np.max(np.abs(Lam))))
        assert float(np.max(np.abs(R.T @ R - Lam), initial=0.0)) < tol and float(np.max(np.abs(R.T @ d - eta), initial=0.0)) < tol
        nodes, xbar = [1, 0], rng.normal(size=(2, 3))
        pts = xbar[[1, 0]] + rng.normal(0, 0.2, (2, 3))           # pts[node]: node 1 is the factor's first
        delta = mm.gaussian_delta(pts, nodes, xbar, dtype)
        r = d - R @ delta
        chi2 = mm.gaussian_chi2(pts, nodes, xbar, eta, Lam, c0, dtype)
        assert abs(float(r @ r - chi2)) < 1e-10 * max(1.0, float(chi2)) and chi2 > -1e-12


def test_heading_wrap():
    xbar = np.array([[0.0, 0.0, 3.1]]); pts = np.array([[0.5, -0.5, -3.1]])
    d = mm.gaussian_delta(pts, [0], xbar)
    assert abs(d[2] - (2 * np.pi - 6.2)) < 1e-15 and d[0] == 0.5 and d[1] == -0.5
    H = np.zeros((3, 3)); g = np.zeros(3)
    Lam = np.diag([1.0, 2.0, 4.0]); eta = np.array([0.1, 0.2, 0.3])
    mm.gaussian_system(H, g, pts, [0], xbar, eta, Lam)
    assert np.array_equal(H, Lam) and np.allclose(g, eta - Lam @ d, rtol=0, atol=1e-15)
