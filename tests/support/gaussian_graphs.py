"""Tiny graphs and helpers shared by the tests of DESIGN.md section 24 (dense Gaussian factors, marginal priors): a seeded odometry
snake with loop closures and a prior, random Gaussian factors of a chosen rank, the graph builder, aprilsam_amd_debug_stage's assembled
system, and the dense numpy model of a whole graph (xyt / xytpos factors + Gaussian factors) with its chi^2 and its normal-equation
residual.  TEST-ONLY."""
import ctypes as C

import numpy as np

from tests.support import marginal_prior_model as mm
from tests.support.normal_eq import linearise


def snake(n, seed, closures=(), prior=0, turn=0.35, noise=0.05):
    """dict(start [n, 3], fa, fb, z [F, 3], W [F, 3, 3]): factor 0 is an xytpos prior on node `prior`, then the odometry, then the closures"""
    rng = np.random.default_rng(seed)
    truth = np.zeros((n, 3))
    for i in range(1, n):
        t = truth[i - 1, 2]
        truth[i] = truth[i - 1] + [np.cos(t), np.sin(t), turn]
    truth[:, 2] = mm.mod2pi(truth[:, 2])
    start = truth + rng.normal(0, noise, truth.shape)
    fa, fb, z, W = [prior], [-1], [truth[prior] + rng.normal(0, 0.01, 3)], [np.diag([100.0, 100.0, 400.0])]
    for a, b in [(i, i + 1) for i in range(n - 1)] + list(closures):
        ca, sa = np.cos(truth[a, 2]), np.sin(truth[a, 2])
        d = truth[b] - truth[a]
        zz = np.array([ca * d[0] + sa * d[1], -sa * d[0] + ca * d[1], mm.mod2pi(d[2])]) + rng.normal(0, 0.02, 3)
        Q = rng.normal(size=(3, 3))
        fa.append(a); fb.append(b); z.append(zz); W.append(Q @ Q.T + np.diag([50.0, 50.0, 300.0]))
    W = np.array(W); W = 0.5 * (W + W.transpose(0, 2, 1))
    return dict(start=start, fa=np.array(fa), fb=np.array(fb), z=np.array(z), W=W)


def random_gaussian(rng, name, k):
    """(xbar [k, 3], eta, Lambda) of rank 3k ("regular"), 3 (k - 1) ("relative": every node tied to the first, nothing absolute) or 0 ("zero")"""
    n = 3 * k
    if name == "regular":
        Q = rng.normal(size=(n, n)); Lam = Q @ Q.T + np.diag(rng.uniform(1, 500, n))
    elif name == "relative":
        J = np.zeros((n - 3, n))
        for i in range(1, k):
            J[3 * i - 3:3 * i, 0:3] = -np.eye(3); J[3 * i - 3:3 * i, 3 * i:3 * i + 3] = np.eye(3) + 0.1 * rng.normal(size=(3, 3))
        Lam = J.T @ np.diag(rng.uniform(5, 300, n - 3)) @ J
    else:
        Lam = np.zeros((n, n))
    Lam = 0.5 * (Lam + Lam.T)
    eta = Lam @ rng.normal(0, 0.3, n)
    xbar = rng.normal(0, 2, (k, 3)); xbar[:, 2] = rng.uniform(-3, 3, k)
    return xbar, eta, Lam


def build(lib, sc, gauss=()):
    """the graph of a snake() scene, plus the Gaussian factors gauss = [(nodes, xbar, eta, Lambda)] behind the scene's own"""
    g = lib.new_graph()
    for s in sc["start"]:
        g.add_node_xyt(s)
    for f in range(len(sc["fa"])):
        if sc["fb"][f] < 0:
            g.add_factor_xytpos(int(sc["fa"][f]), sc["z"][f], sc["W"][f])
        else:
            g.add_factor_xyt(int(sc["fa"][f]), int(sc["fb"][f]), sc["z"][f], sc["W"][f])
    for nodes, xbar, eta, Lam in gauss:
        g.add_factor_gaussian(nodes, xbar, eta, Lam)
    return g


def assembled(lib, g, p):
    """aprilsam_amd_debug_stage what = 1: the assembled (A [3N, 3N], B [3N]) in node coordinates, linearised at the current states"""
    lib.dll.aprilsam_amd_debug_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    n = 3 * g.n_nodes
    out = np.full(n * n + n, np.nan)
    rc = lib.dll.aprilsam_amd_debug_stage(C.cast(g.ptr, C.c_void_p), C.cast(p.ptr, C.c_void_p), 1, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, (rc, lib.last_error())
    return out[:n * n].reshape(n, n), out[n * n:]


def model_system(sc, lp, gauss=(), lam=0.0, dtype=np.float64, only=None):
    """(A, B) of the scene's factors and the Gaussian factors at lp, with lam on the diagonal: what a step assembles"""
    H, g = mm.dense_system(lp, sc["fa"], sc["fb"], sc["z"], sc["W"], dtype, only=only)
    for nodes, xbar, eta, Lam in gauss:
        mm.gaussian_system(H, g, lp, nodes, xbar, eta, Lam)
    H[np.diag_indices_from(H)] += dtype(lam)
    return H, g


def model_step(sc, lp, gauss=(), lam=0.0, dtype=np.float64):
    A, B = model_system(sc, lp, gauss, lam, dtype)
    return mm.solve_spd(A, B, dtype).reshape(-1, 3)


def model_chi2(sc, st, gauss=(), halves=True):
    """april_graph_chi2's sum at the states st (halves: 0.5 r'Wr for xyt factors, april_graph.c:79-98) or LM's objective (halves=False);
    a Gaussian factor's term is c0 - 2 eta'delta + delta'Lambda delta with c0 of the longdouble square-root form"""
    _, _, r = linearise(st, sc["fa"], sc["fb"], sc["z"])
    t = np.einsum("ni,nij,nj->n", r, sc["W"], r)
    total = float(np.sum(np.where(sc["fb"] >= 0, 0.5 if halves else 1.0, 1.0) * t))
    terms = []
    for nodes, xbar, eta, Lam in gauss:
        _, _, c0 = mm.sqrt_form(eta, Lam, np.longdouble)
        terms.append(float(mm.gaussian_chi2(st, nodes, xbar, eta, Lam, c0, np.longdouble)))
    return total + sum(terms), terms


def normal_eq_rel(sc, lp, dx, gauss=(), lam=0.0):
    """max |A dx - B| over the size of the right-hand side's terms (sum_f |J_f'W_f r_f| per component, the Gaussian factors' |eta| and
    |Lambda delta| included): tests/support/normal_eq.py's measure, on the dense model"""
    A, B = model_system(sc, lp, gauss, lam, np.longdouble)
    res = A @ np.asarray(dx, np.longdouble).reshape(-1) - B
    N = len(lp)
    Ja, Jb, r = linearise(lp, sc["fa"], sc["fb"], sc["z"])
    Wr = np.einsum("nij,nj->ni", sc["W"], r)
    scale = np.zeros((N, 3))
    np.add.at(scale, sc["fa"], np.abs(np.einsum("nji,nj->ni", Ja, Wr)))
    b = sc["fb"] >= 0
    np.add.at(scale, sc["fb"][b], np.abs(np.einsum("nji,nj->ni", Jb, Wr))[b])
    scale = scale.reshape(-1)
    for nodes, xbar, eta, Lam in gauss:
        d = mm.gaussian_delta(lp, nodes, xbar)
        scale[mm._rows(nodes)] += np.abs(eta) + np.abs(Lam) @ np.abs(d)
    return float(np.max(np.abs(res)) / np.max(scale))
