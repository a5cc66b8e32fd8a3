"""Gating of range / bearing / range-bearing candidates and their nearest-neighbour association against landmarks on the GPU
(aprilsam_amd_gate_polar, aprilsam_amd_associate_polar) against the numpy model (tests/support/polar_gate_model.py)
with Sigma the dense inverse of the model's system; against aprilsam_amd_gate_xyt on xyt twins; after batch, resident and incremental
steps, with fixed nodes, behind five kernel-path option sets; bitwise repeatability, non-interference and every refusal.
Tolerance: the project's 1e-9, as tests/test_gpu_gating.py::test_gate_matches_the_model applies it to d2 and S."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import host
from tests.support import fixed_model as fm
from tests.support import gate_model
from tests.support import polar_gate_model as pg
from tests.support import polar_model as pm
from tests.support.kernel_paths import KERNEL_PATHS

pytestmark = pytest.mark.gpu
GATE_RTOL = 1e-9
G1, G2 = pg.CHI2_1_999, pg.CHI2_2_999


def _check(d2, S, md2, mS, what, ok=None):
    """test_gate_matches_the_model's bounds: d2 to 1e-9 of the largest and of each entry, S to 1e-9 of its largest entry"""
    d2, md2, S, mS = np.asarray(d2), np.asarray(md2), np.asarray(S), np.asarray(mS)
    keep = np.ones(len(d2), bool) if ok is None else np.asarray(ok, bool)
    e_d = np.abs(d2 - md2)[keep]
    worst_d = (e_d / np.abs(md2[keep])).max(); worst_S = np.abs(S[keep] - mS[keep]).max() / np.abs(mS[keep]).max()
    print(f"{what}: worst deviation of d2 {worst_d:.3e}, of S {worst_S:.3e}")
    assert e_d.max() < GATE_RTOL * np.abs(md2[keep]).max() and (e_d <= GATE_RTOL * np.abs(md2[keep]) + 1e-300).all(), (what, worst_d)
    assert worst_S < GATE_RTOL, (what, worst_S)


def _cand(kind, zz):
    """(kind, z, W) from a range-bearing reading zz, with the generator's information (the range-bearing W correlated)"""
    if kind == pm.RANGE:
        return kind, np.array(zz[:1]), np.array([[1 / pm.SIGMA_RHO ** 2]])
    if kind == pm.BEARING:
        return kind, np.array(zz[1:]), np.array([[1 / pm.SIGMA_BETA ** 2]])
    cr = 0.3 / (pm.SIGMA_RHO * pm.SIGMA_BETA)
    return kind, np.array(zz), np.array([[1 / pm.SIGMA_RHO ** 2, cr], [cr, 1 / pm.SIGMA_BETA ** 2]])


def _candidates(states, observers, targets, n, seed, kinds=(pm.RANGE_BEARING, pm.RANGE, pm.BEARING)):
    """n candidates, the kinds cycling: a random observer, a random other node, z a few sigma off what the states predict"""
    rng = np.random.default_rng(seed)
    a, b, cands = [], [], []
    while len(a) < n:
        i, j = int(rng.choice(observers)), int(rng.choice(targets))
        if i == j:
            continue
        zz = pm.h(pm.RANGE_BEARING, pm.rel(states[i], states[j])[0]) + rng.normal(0, [0.05, 0.03])
        a.append(i); b.append(j); cands.append(_cand(kinds[len(a) % len(kinds)], zz))
    return np.array(a, np.int32), np.array(b, np.int32), cands


def _gate_against_model(g, p, Sigma, a, b, cands, what):
    kind, z, W = host.polar_candidates(cands)
    bad, d2, S = g.gate_polar(p, a, b, kind, z, W)
    ok, md2, mS = pg.gate(g.states(), a, b, cands, pg.joint_blocks(Sigma, a, b))
    assert bad == 0 and ok.all()
    _check(d2, S, md2, pg.padded(mS), what)
    return d2, S


@pytest.fixture(scope="module")
def small():
    """6 poses + 3 landmarks, all three kinds"""
    return pm.snake(3, 3, seed=7, n_rows=2)


@pytest.fixture(scope="module")
def medium():
    """K = 6, L = 8"""
    return pm.snake(6, 8, seed=2)


# ---- 1. gate_polar against the model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["small", "medium"])
@pytest.mark.parametrize("how", ["batch", "resident"])
def test_gate_polar_against_the_model(lib, small, medium, which, how):
    d = small if which == "small" else medium
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    assert p.c.tikhanov == pm.TIKHANOV
    if how == "batch":
        g.cholesky(p)
    else:
        g.batch_resident(p, 3)
    assert p.stats()["not_spd"] == 0
    Sigma = pg.dense_sigma(g.l_points(), d["plain"], d["polars"], pm.TIKHANOV)
    n, N = d["n_poses"], len(d["start"])
    assert not np.array_equal(g.states(), g.l_points())                     # (the residual is taken at the states, Sigma at the l_points)
    a, b, cands = _candidates(g.states(), np.arange(n), np.arange(N), 40, 3)
    a, b, cands = np.r_[a, a[:3]], np.r_[b, b[:3]], cands + [cands[1], cands[2], cands[0]]      # pairs named twice, by other candidates
    assert (b >= n).any() and (b < n).any()                                 # landmarks and poses
    _gate_against_model(g, p, Sigma, a, b, cands, f"{which} after a {how} run")
    p.destroy(); g.destroy()


def _grown(lib, d, calls):
    """the snake grown through april_graph_cholesky_inc, as tests/test_gpu_polar.py grows it: one call after every pose's odometry and one
    after every polar factor; a new landmark arrives with its first sighting and its heading prior.  The first call is a batch step.
    -> (g, p, plain, polars in the grown graph's ids, nodes under Tikhonov, landmarks added by incremental steps)"""
    fa, fb, z, W = d["plain"]
    n = d["n_poses"]
    g = lib.new_graph(); p = lib.new_param(nthreshold=100)
    node, out = {}, dict(fa=[], fb=[], z=[], W=[], polars=[], done=0, n_batch=0, late=[], poses=[], lms=[])

    def step():
        if out["done"] == 0:
            g.cholesky(p); out["n_batch"] = g.n_nodes
        else:
            p.c.batch_time = 1e300
            bt = p.c.batch_time
            g.cholesky_inc(p)
            if p.c.batch_time != bt:
                out["n_batch"] = g.n_nodes
        assert p.stats()["not_spd"] == 0 and lib.last_error()[0] == 0, (out["done"], lib.last_error())
        out["done"] += 1

    def plain(a, b, zz, WW):
        out["fa"].append(a); out["fb"].append(b); out["z"].append(np.asarray(zz, float)); out["W"].append(np.asarray(WW, float).reshape(9))
        if b < 0:
            g.add_factor_xytpos(a, zz, np.asarray(WW, float).reshape(3, 3))
        else:
            g.add_factor_xyt(a, b, zz, np.asarray(WW, float).reshape(3, 3))

    lib.clear_error()
    for i in range(n):
        for what, k in d["events"][i]:
            if out["done"] >= calls:
                break
            if what == "node" and k < n:
                pa = g.states_of(node[k - 1]) if k else None
                node[k] = g.add_node_xyt(d["start"][0] if k == 0 else _compose(pa, z[k]))
                out["poses"].append(node[k])
            elif what == "plain":
                plain(node[int(fa[k])], node[int(fb[k])] if fb[k] >= 0 else -1, z[k], W[k])
                step()
            elif what == "polar":
                kind, a, b, zz, WW = d["polars"][k]
                if b not in node:
                    pa = g.states_of(node[a])
                    node[b] = g.add_node_xyt([pa[0] + zz[0] * np.cos(pa[2] + zz[1]), pa[1] + zz[0] * np.sin(pa[2] + zz[1]), 0.0])
                    out["lms"].append(node[b])
                    if out["done"] > 0:
                        out["late"].append(node[b])
                    plain(node[b], -1, [0.0, 0.0, 0.0], np.diag([0.0, 0.0, 1.0]))      # the heading prior of include/aprilsam_amd.h
                g.add_factor_polar(kind, node[a], node[b], zz, WW)
                out["polars"].append((kind, node[a], node[b], zz, WW))
                step()
    out["plain"] = (np.array(out["fa"], np.int64), np.array(out["fb"], np.int64), np.array(out["z"]), np.array(out["W"]))
    return g, p, out


def _compose(pa, z):
    c, s = np.cos(pa[2]), np.sin(pa[2])
    v = pa[2] + z[2]
    return np.array([pa[0] + c * z[0] - s * z[1], pa[1] + s * z[0] + c * z[1], (v + np.pi) % (2 * np.pi) - np.pi])


def test_gate_polar_after_incremental_steps(lib, medium):
    g, p, o = _grown(lib, medium, 21)                                        # one batch call and 20 incremental ones
    assert o["done"] == 21 and len(o["late"]) >= 1 and o["n_batch"] < g.n_nodes
    # the system of an incremental run: Tikhonov on the nodes of the last batch step only (tests/support/sigma_compare.py)
    A, _ = pm.system(g.l_points(), o["plain"], o["polars"], 0.0)
    A = A.toarray(); k = 3 * o["n_batch"]
    A[np.arange(k), np.arange(k)] += pm.TIKHANOV
    Sigma = np.linalg.inv(A)
    a, b, cands = _candidates(g.states(), o["poses"], o["poses"] + o["lms"], 24, 5)
    a2, b2, cands2 = _candidates(g.states(), o["poses"], o["late"], 6, 6)   # ... and the landmarks the incremental steps added
    a, b, cands = np.r_[a, a2], np.r_[b, b2], cands + cands2
    _gate_against_model(g, p, Sigma, a, b, cands, "after 20 incremental steps")
    _assoc_against_model(g, p, Sigma, o["poses"][-1], cands[:5], np.array(o["lms"], np.int32), "association after 20 incremental steps")
    p.destroy(); g.destroy()


# ---- 2. gate_polar against gate_xyt -------------------------------------------------------------------------------------------------
def test_gate_polar_against_gate_xyt_twins(lib, medium):
    """S_polar = G S_xyt[:2, :2] G' for the twin with the same z in Cartesian form, W_xyt = blockdiag(G' W G, w_theta) and a zero heading
    residual, so d2_polar is the d2 of the twin's first two rows with the residual in polar coordinates; for the twin whose first two
    residuals are G^-1 r_p (the Cartesian form to first order in r_p) it is r2' S2^-1 r2 with r2 the xyt residual itself.  The
    projections are done here"""
    d = medium
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    g.cholesky(p)
    st = g.states()
    n, N = d["n_poses"], len(st)
    a, b, cands = _candidates(st, np.arange(n), np.arange(N), 24, 9, kinds=(pm.RANGE_BEARING,))
    kind, z, W = host.polar_candidates(cands)
    bad, d2p, Sp = g.gate_polar(p, a, b, kind, z, W)
    assert bad == 0
    tw = [pg.xyt_twin(c[1], c[2], st[i], st[j], w_theta=7.0) for c, i, j in zip(cands, a, b)]
    _, Sx = g.gate_xyt(p, a, b, np.array([t[0] for t in tw]), np.array([t[1] for t in tw]))
    want_S, want_d2, want_lin = [], [], []
    for k, (c, i, j) in enumerate(zip(cands, a, b)):
        G = tw[k][2]
        q = gate_model.predict(st[i], st[j])
        rp = pm.residual(pm.RANGE_BEARING, c[1], q[:2])
        S2 = np.asarray(Sx)[k].reshape(3, 3)[:2, :2]
        want_S.append(G @ S2 @ G.T)
        want_d2.append(rp @ np.linalg.solve(want_S[-1], rp))
        r2 = np.linalg.solve(G, rp)                                           # the first two residuals of the linearised twin z3 = (q + G^-1 r_p, q2)
        want_lin.append(r2 @ np.linalg.solve(S2, r2))
    _check(d2p, Sp, want_d2, want_S, "gate_polar against gate_xyt's first two rows in polar coordinates")
    _check(d2p, Sp, want_lin, want_S, "gate_polar against the linearised twin's r2' S2^-1 r2")
    p.destroy(); g.destroy()


# ---- 3. a landmark standing on its observer -------------------------------------------------------------------------------------------
def test_landmark_on_its_observer_is_unavailable(lib, small):
    d = small
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    g.cholesky(p)
    n = d["n_poses"]
    a, b, cands = _candidates(g.states(), np.arange(n), np.arange(n, n + 3), 9, 1)
    kind, z, W = host.polar_candidates(cands)
    _, d2_0, S_0 = g.gate_polar(p, a, b, kind, z, W)
    st = g.states()
    k = 4
    others = [i for i in range(9) if b[i] != b[k]]
    assert others
    g.set_state(int(b[k]), [st[a[k], 0], st[a[k], 1], 0.4])                   # rho^2 == 0 for candidate k (and whoever else names that pair)
    hit = [i for i in range(9) if (a[i], b[i]) == (a[k], b[k])]
    bad, d2, S = g.gate_polar(p, a, b, kind, z, W)
    assert bad == len(hit)
    for i in hit:
        m = pm.rows(kind[i])
        assert np.isnan(d2[i]) and np.isnan(S[i].ravel()[:m * m]).all()
    assert d2[others].tobytes() == d2_0[others].tobytes() and S[others].tobytes() == S_0[others].tobytes()
    r = g.associate_polar(p, int(a[k]), kind[:3], z[:3], W[:3], np.arange(n, n + 3), G1, G2)
    col = int(b[k]) - n
    assert r["unavailable"] == 3 and np.isnan(r["d2"][:, col]).all() and np.all(r["best"] != col) and np.isfinite(np.delete(r["d2"], col, 1)).all()
    p.destroy(); g.destroy()


# ---- 4. associate_polar ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pinned(lib):
    """the case tests/test_polar_gate_model.py pins on the CPU, after one batch step from the model's solved states"""
    c = pg.association_case()
    d = c["d"]
    g = pm.build(lib, c["x"], d["plain"], d["polars"]); p = lib.new_param()
    g.cholesky(p)
    Sigma = pg.dense_sigma(g.l_points(), d["plain"], d["polars"], pm.TIKHANOV)
    yield c, g, p, Sigma
    p.destroy(); g.destroy()


def _assoc_against_model(g, p, Sigma, observer, obs, lms, what, g1=G1, g2=G2):
    kind, z, W = host.polar_candidates(obs)
    r = g.associate_polar(p, observer, kind, z, W, lms, g1, g2)
    m = pg.associate(g.states(), observer, obs, lms, pg.joint_blocks(Sigma, [observer] * len(lms), lms), g1, g2)
    assert r["unavailable"] == m["unavailable"] == 0
    assert np.array_equal(r["best"], m["best"]), (what, r["best"], m["best"])
    e = np.abs(r["d2"] - m["d2"]) / np.abs(m["d2"])
    print(f"{what}: worst deviation of the matrix {e.max():.3e}")
    assert e.max() <= GATE_RTOL
    for key in ("d2_best", "d2_second"):
        fin = np.isfinite(m[key])
        assert np.array_equal(np.isinf(r[key]), ~fin) and (np.abs(r[key][fin] - m[key][fin]) <= GATE_RTOL * np.abs(m[key][fin])).all(), (what, key)
    return r, m


def test_associate_on_the_pinned_case(pinned):
    c, g, p, Sigma = pinned
    r, m = _assoc_against_model(g, p, Sigma, c["observer"], c["obs"], c["landmarks"], "pinned case")
    assert np.array_equal(r["best"], c["truth_idx"])                          # every observation finds its landmark
    # the matrix is gate_polar on the expanded list, bit for bit
    kind, z, W = host.polar_candidates(c["obs"])
    mm, L = len(c["obs"]), len(c["landmarks"])
    a = np.full(mm * L, c["observer"], np.int32); b = np.tile(c["landmarks"], mm)
    bad, d2, _ = g.gate_polar(p, a, b, np.repeat(kind, L), np.repeat(z, L, 0), np.repeat(W, L, 0))
    assert bad == 0 and d2.tobytes() == r["d2"].tobytes()
    # without the matrix: the same answers
    r2 = g.associate_polar(p, c["observer"], kind, z, W, c["landmarks"], G1, G2, matrix=False)
    assert r2["d2"] is None and all(r2[k].tobytes() == r[k].tobytes() for k in ("best", "d2_best", "d2_second"))
    # m = 1
    r1 = g.associate_polar(p, c["observer"], kind[2:3], z[2:3], W[2:3], c["landmarks"], G1, G2)
    assert r1["best"][0] == r["best"][2] and r1["d2"].tobytes() == r["d2"][2:3].tobytes() and r1["d2_second"][0] == r["d2_second"][2]


def test_associate_edge_cases(pinned):
    c, g, p, Sigma = pinned
    kind, z, W = host.polar_candidates(c["obs"])
    lms, o = c["landmarks"], c["observer"]
    full = g.associate_polar(p, o, kind, z, W, lms, G1, G2)
    # L = 1: no second; L = 0: nothing to match
    r = g.associate_polar(p, o, kind, z, W, lms[:1], G1, G2)
    assert np.all(np.isposinf(r["d2_second"])) and r["d2_best"].tobytes() == np.ascontiguousarray(full["d2"][:, 0]).tobytes()
    assert np.array_equal(r["best"], np.where(full["d2"][:, 0] <= np.where(kind == pm.RANGE_BEARING, G2, G1), 0, -1)) and r["best"][c["truth_idx"] == 0].tolist() == [0]
    r = g.associate_polar(p, o, kind, z, W, lms[:0], G1, G2)
    assert r["unavailable"] == 0 and np.all(r["best"] == -1) and np.all(np.isposinf(r["d2_best"])) and np.all(np.isposinf(r["d2_second"]))
    assert g.associate_polar(p, o, kind[:0], z[:0], W[:0], lms, G1, G2)["unavailable"] == 0
    # a landmark listed twice resolves to the lower index, and its second-smallest d2 is the smallest again
    twice = np.r_[lms, lms[:4]].astype(np.int32)
    r, _ = _assoc_against_model(g, p, Sigma, o, c["obs"], twice, "landmarks listed twice")
    assert np.array_equal(r["best"], c["truth_idx"])
    dup = c["truth_idx"] < 4
    assert dup.any() and r["d2_second"][dup].tobytes() == r["d2_best"][dup].tobytes()
    assert r["d2"][:, 8:].tobytes() == np.ascontiguousarray(r["d2"][:, :4]).tobytes()
    # far from every landmark: a new landmark, with a finite distance to the nearest
    far = [(pm.RANGE_BEARING, np.array([40.0, 0.3]), c["obs"][0][2]), (pm.RANGE, np.array([55.0]), np.array([[2500.0]]))]
    r, _ = _assoc_against_model(g, p, Sigma, o, far, lms, "far observations")
    assert np.all(r["best"] == -1) and np.all(np.isfinite(r["d2_best"])) and r["d2_best"][0] > G2 and r["d2_best"][1] > G1
    # the gate is the caller's: nothing passes a gate of 0, everything a huge one
    r0 = g.associate_polar(p, o, kind, z, W, lms, 0.0, 0.0)
    assert np.all(r0["best"] == -1) and r0["d2_best"].tobytes() == full["d2_best"].tobytes()
    r1 = g.associate_polar(p, o, kind[:2], z[:2], W[:2], lms, 1e300, 0.0)     # (observation 0 has two rows, observation 1 one)
    assert r1["best"][0] == -1 and r1["best"][1] == c["truth_idx"][1]


@pytest.fixture(scope="module")
def many(lib, medium):
    """the 36-pose snake with 300 landmarks: a thread walks more than one landmark, the tree merges partial pairs"""
    d = medium
    n = d["n_poses"]
    truth, start, polars = pm.with_landmarks(d["truth"][:n], d["start"][:n], 300, seed=4)
    g = pm.build(lib, start, d["plain"], polars); p = lib.new_param()
    g.cholesky(p); g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    Sigma = pg.dense_sigma(g.l_points(), d["plain"], polars, pm.TIKHANOV)
    yield truth, g, p, Sigma, n
    p.destroy(); g.destroy()


def test_associate_against_300_landmarks(many):
    truth, g, p, Sigma, n = many
    rng = np.random.default_rng(8)
    observer = n - 1
    lms = np.arange(n, n + 300, dtype=np.int32)
    near = [l for l in lms if np.hypot(*pm.rel(truth[observer], truth[l])[0]) < 2.5]
    obs, kinds = [], (pm.RANGE_BEARING, pm.RANGE, pm.BEARING)
    for k in range(33):                                                       # m = 33
        zz = pm.h(pm.RANGE_BEARING, pm.rel(truth[observer], truth[near[k % len(near)]])[0]) + rng.normal(0, [pm.SIGMA_RHO, pm.SIGMA_BETA])
        obs.append(_cand(kinds[k % 3], zz))
    r, m = _assoc_against_model(g, p, Sigma, observer, obs, lms, "300 landmarks, 33 observations")
    assert (r["best"] >= 256).any() and (r["best"] >= 0).sum() >= 20 and np.all(np.isfinite(r["d2_second"]))
    # a permuted landmark list: the same landmarks are found
    perm = rng.permutation(300)
    kind, z, W = host.polar_candidates(obs)
    rp = g.associate_polar(p, observer, kind, z, W, lms[perm], G1, G2)
    found = r["best"] >= 0
    assert np.array_equal(rp["best"] >= 0, found) and np.array_equal(lms[perm][rp["best"][found]], lms[r["best"][found]])
    assert rp["d2_best"].tobytes() == r["d2_best"].tobytes() and rp["d2_second"].tobytes() == r["d2_second"].tobytes()


# ---- 5. fixed nodes ------------------------------------------------------------------------------------------------------------------------
def test_fixed_landmark_and_fixed_observer(lib, small):
    d = small
    n = d["n_poses"]
    fixed = (2, n + 1)                                                        # an observer and a landmark
    g = fm.build(lib, d["start"], d["plain"], d["polars"], fixed=fixed); p = lib.new_param()
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    A, _ = fm.system(g.l_points(), d["plain"], d["polars"], lam=pm.TIKHANOV)
    Sigma = fm.conditional_covariance(A, fixed)                               # Sigma_Phi = 0
    a = np.array([0, 2, 2, 4, 1], np.int32); b = np.array([n + 1, n, n + 1, n + 2, n + 1], np.int32)      # (free, fixed) (fixed, free) (fixed, fixed) (free, free)
    st = g.states()
    kinds = (pm.RANGE, pm.BEARING, pm.RANGE_BEARING, pm.RANGE_BEARING, pm.BEARING)
    cands = [_cand(k, pm.h(pm.RANGE_BEARING, pm.rel(st[i], st[j])[0]) + [0.03, -0.02]) for k, i, j in zip(kinds, a, b)]
    d2, S = _gate_against_model(g, p, Sigma, a, b, cands, "fixed nodes")
    Winv = np.linalg.inv(cands[2][2])
    assert np.abs(S[2].ravel()[:Winv.size] - Winv.ravel()).max() <= 1e-12 * np.abs(Winv).max()      # between two fixed nodes: S = W^-1
    obs = [cands[0], cands[4], cands[2]]
    lms = np.arange(n, n + 3, dtype=np.int32)
    _assoc_against_model(g, p, Sigma, 0, obs, lms, "association with a fixed landmark")
    _assoc_against_model(g, p, Sigma, 2, obs, lms, "association from a fixed observer")
    p.destroy(); g.destroy()


# ---- 6. repeatability and non-interference ------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_steps_are_unaffected(lib, medium):
    d = medium
    n, N = d["n_poses"], len(d["start"])
    a, b, cands = _candidates(d["start"], np.arange(n), np.arange(N), 30, 6)
    kind, z, W = host.polar_candidates(cands)
    lms = np.arange(n, N, dtype=np.int32)
    runs = []
    for with_calls in (False, True):
        g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
        snaps = []
        for it in range(4):
            g.cholesky(p)
            if with_calls:
                r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
                x1 = g.gate_polar(p, a, b, kind, z, W); x2 = g.gate_polar(p, a, b, kind, z, W)
                assert x1[0] == x2[0] and x1[1].tobytes() == x2[1].tobytes() and x1[2].tobytes() == x2[2].tobytes()
                y1 = g.associate_polar(p, n - 1, kind[:7], z[:7], W[:7], lms, G1, G2); y2 = g.associate_polar(p, n - 1, kind[:7], z[:7], W[:7], lms, G1, G2)
                assert all(y1[k].tobytes() == y2[k].tobytes() for k in ("best", "d2_best", "d2_second", "d2"))
                assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0          # no selected inversion runs
            snaps.append(np.concatenate([g.states(), g.deltas(), g.l_points()]).tobytes())
        runs.append(snaps)
        p.destroy(); g.destroy()
    assert runs[0] == runs[1]


# ---- 7. kernel paths -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def landmark_case():
    """the 700-pose random graph with 20 landmarks of tests/test_gpu_polar.py, its dense Sigma at the start, and 60 candidates"""
    from tests.test_gpu_polar import _landmark_graph
    x, plain, polars = _landmark_graph()
    Sigma = pg.dense_sigma(x, plain, polars, pm.TIKHANOV)
    N = len(x)
    a, b, cands = _candidates(x, np.arange(N - 20), np.arange(N - 20, N), 60, 12)
    return x, plain, polars, Sigma, a, b, cands


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


@pytest.mark.parametrize("opts", [KERNEL_PATHS[0], KERNEL_PATHS[10], KERNEL_PATHS[27], dict(pool_guard=64), dict(pool_poison=1)], ids=_ids)
def test_behind_every_kernel_path(lib, landmark_case, opts):
    x, plain, polars, Sigma, a, b, cands = landmark_case
    with lib.options(**opts):
        g = pm.build(lib, x, plain, polars); p = lib.new_param()
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0 and np.array_equal(g.l_points(), x)
        _gate_against_model(g, p, Sigma, a, b, cands, _ids(opts))
        p.destroy(); g.destroy()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing_and_leaves_the_param_alone(lib, small):
    from tests.support.asym_scenarios import batch_graph
    from tests.test_polar_gate_host import REFUSALS_ASSOC, REFUSALS_GATE, _calls
    d = small
    ref = pm.build(lib, d["start"], d["plain"], d["polars"]); pr = lib.new_param()
    ref.cholesky(pr); ref.cholesky(pr)
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    gate, assoc = _calls(lib, g, p)
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    N = g.n_nodes

    def refused(call, code, **ch):
        lib.clear_error()
        assert call(**ch) == (code, True) and lib.last_error()[0] == code, (code, ch)
    refused(gate, -1); refused(assoc, -1)                                     # a fresh param: no retained factor
    g.cholesky(p)
    r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    for ch, code in REFUSALS_GATE:
        refused(gate, code, **ch)
    for ch, code in REFUSALS_ASSOC:
        refused(assoc, code, **ch)
    # ids out of range of the factorised system, then of the graph
    refused(gate, -13, b=i32([2, N])); refused(gate, -13, a=i32([-1, 1]))
    refused(assoc, -13, observer=N); refused(assoc, -13, observer=-1); refused(assoc, -13, lm=i32([1, 2, N])); refused(assoc, -13, lm=i32([1, -3, 2]))
    new = g.add_node_xyt([9.0, 9.0, 0.0])                                     # (added since the last solver call)
    assert new == N
    refused(gate, -13, b=i32([2, new])); refused(assoc, -13, lm=i32([1, 2, new])); refused(assoc, -13, observer=new)
    # a sharded param, and a factorised graph with an asymmetric information matrix
    dll = lib.dll
    dll.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    dll.aprilsam_amd_shard_end.argtypes = [C.c_void_p]
    from tests.support.marginal_cases import case_arrays
    g3 = lib.new_graph(); g3.build_from_arrays(*case_arrays(lib, "lattice24")); p3 = lib.new_param()
    g3.cholesky(p3)
    assert dll.aprilsam_amd_shard_begin(C.cast(g3.ptr, C.c_void_p), C.cast(p3.ptr, C.c_void_p), 0, 1) == 0
    gate3, assoc3 = _calls(lib, g3, p3)
    refused(gate3, -12); refused(assoc3, -12)
    dll.aprilsam_amd_shard_end(C.cast(p3.ptr, C.c_void_p))
    g4 = lib.new_graph(); g4.build_from_arrays(*batch_graph()); p4 = lib.new_param()
    g4.cholesky(p4)
    gate4, assoc4 = _calls(lib, g4, p4)
    refused(gate4, -12); refused(assoc4, -12)
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0
    p.destroy(); g.destroy()                                                  # (that graph has grown by a node)
    # the next solver call on a param that saw refusals of every stage since its last one: the bits of an untouched param
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    gate, assoc = _calls(lib, g, p)
    g.cholesky(p)
    for ch, code in REFUSALS_GATE[:3] + REFUSALS_GATE[-3:]:
        refused(gate, code, **ch)
    for ch, code in REFUSALS_ASSOC[-5:]:
        refused(assoc, code, **ch)
    refused(gate, -13, b=i32([2, N])); refused(assoc, -13, lm=i32([1, 2, N]))
    g.cholesky(p)
    assert g.states().tobytes() == ref.states().tobytes()
    assert g.gate_polar(p, [0], [N - 1], [pm.RANGE], [[1.0, 0]], [[4.0, 0, 0, 0]])[1].tobytes() == \
        ref.gate_polar(pr, [0], [N - 1], [pm.RANGE], [[1.0, 0]], [[4.0, 0, 0, 0]])[1].tobytes()
    for x in (p, g, pr, ref, p3, g3, p4, g4):
        x.destroy()
