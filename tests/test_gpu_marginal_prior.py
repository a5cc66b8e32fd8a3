"""aprilsam_amd_marginal_prior and aprilsam_amd_graph_marginalize on the GPU: keep, xbar, eta and Lambda against
the dense numpy model in longdouble (tests/support/marginal_prior_model.py) -- chain ends, mid-chain poses, non-adjacent and adjacent
removed sets, robust-weighted, max-mixture, polar, host-evaluated and Gaussian factors touching the removed set, |M| + |B| = 40 and 41;
the reduced graph's step and marginals against the full graph's; LM, GNC and the resident loop on the reduced graph; every refusal.

Tolerances: ten times what the float64 model deviates from the longdouble model on the same input (DESIGN.md section 24 records the
figures the tests print)."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import abi
from tests.support import gaussian_graphs as gg
from tests.support import marginal_prior_model as mm

pytestmark = pytest.mark.gpu
LAM = 1e-4
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _dev(a64, ald):
    return float(np.max(np.abs(np.asarray(a64, np.longdouble) - ald), initial=0.0))


def _raw(lib, g, p, remove, cap):
    """the C call on NaN / -7 prefilled outputs: (rc, n_keep, keep, xbar, eta, Lambda)"""
    rm = np.ascontiguousarray(remove, np.int32)
    nk = C.c_int(-7); keep = np.full(max(cap, 1), -7, np.int32)
    xbar = np.full(3 * max(cap, 1), np.nan); eta = np.full(3 * max(cap, 1), np.nan); L = np.full(9 * max(cap, 1) ** 2, np.nan)
    rc = lib.dll.aprilsam_amd_marginal_prior(g.ptr, p.ptr, len(rm), rm.ctypes.data_as(_ip), cap, C.byref(nk), keep.ctypes.data_as(_ip),
                                            xbar.ctypes.data_as(_dp), eta.ctypes.data_as(_dp), L.ctypes.data_as(_dp))
    return rc, nk.value, keep, xbar, eta, L


def _untouched(out):
    rc, nk, keep, xbar, eta, L = out
    return nk == -7 and (keep == -7).all() and np.isnan(xbar).all() and np.isnan(eta).all() and np.isnan(L).all()


def _check(lib, tag, got, sc, lp, remove, gauss=()):
    """keep, xbar, eta, Lambda of the device against the model on the effective scene sc (W and z as the slots were linearised); the
    Gaussian factors of `gauss` touch M and count as they stand"""
    def extra(H, g):
        for nodes, xbar, eta, Lam in gauss:
            mm.gaussian_system(H, g, lp, nodes, xbar, eta, Lam)
    more = [n for ga in gauss for n in ga[0]]
    m64 = mm.marginal_prior(lp, sc["fa"], sc["fb"], sc["z"], sc["W"], remove, np.float64, extra if gauss else None, more)
    ml = mm.marginal_prior(lp, sc["fa"], sc["fb"], sc["z"], sc["W"], remove, np.longdouble, extra if gauss else None, more)
    B = list(ml[0])
    assert list(got[0]) == B, (got[0], B)
    assert np.array_equal(got[1], lp[B])                                                    # the linearisation point, bit for bit
    assert np.array_equal(got[3], got[3].T)
    for what, k in (("eta", 2), ("Lambda", 3)):
        allowed, err = 10 * _dev(m64[k], ml[k]), _dev(got[k], ml[k])
        print(f"marginal prior {tag} {what}: |device - longdouble| = {err:.3e}, allowed 10 x |float64 - longdouble| = {allowed:.3e}")
        assert err <= allowed, (tag, what, err, allowed)
    return ml


# ---- 5. the prior against the model -----------------------------------------------------------------------------------------------------
PLAIN = {
    "chain_end_with_prior": (8, [], [0]),                       # |M| = 1, |B| = 1: the xytpos prior sits on the removed pose
    "mid_chain": (8, [], [4]),                                  # |M| = 1, |B| = 2: Lambda has rank 3
    "three_non_adjacent": (12, [(0, 11), (2, 9)], [3, 6, 9]),
    "two_adjacent_with_closure": (12, [(0, 11), (5, 10), (2, 8)], [4, 5]),
    "unordered": (12, [(0, 11), (5, 10), (2, 8)], [8, 2, 5]),
}


@pytest.mark.parametrize("case", list(PLAIN))
def test_prior_against_the_model(lib, case):
    n, closures, remove = PLAIN[case]
    sc = gg.snake(n, 61, closures)
    g = gg.build(lib, sc); p = lib.new_param()
    g.cholesky(p)
    lp = g.l_points()
    got = g.marginal_prior(p, remove)
    ml = _check(lib, case, got, sc, lp, remove)
    again = g.marginal_prior(p, remove)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))                       # two calls: the same bits
    if case == "mid_chain":
        assert mm.pivoted_cholesky(got[3])[1] == 3
    if case == "chain_end_with_prior":
        assert list(got[0]) == [1] and mm.pivoted_cholesky(got[3])[1] == 3
    # no lambda in it: the same call under another tikhanov gives the same prior to rounding
    q = lib.new_param(); q.c.tikhanov = 10.0
    g.set_all_states(lp)
    g.cholesky(q)
    other = g.marginal_prior(q, remove)
    assert _dev(other[3], ml[3]) <= 10 * _dev(mm.marginal_prior(lp, sc["fa"], sc["fb"], sc["z"], sc["W"], remove)[3], ml[3])
    for x in (p, q):
        x.destroy()
    g.destroy()


def test_weighted_selected_polar_host_and_gaussian_factors_count_as_linearised(lib):
    sc = gg.snake(12, 62, closures=[(0, 11)])
    rng = np.random.default_rng(63)
    F0 = len(sc["fa"])
    W = np.diag([80.0, 80.0, 300.0])

    def meas(a, b, off=(0, 0, 0)):
        pa, pb = sc["start"][a], sc["start"][b]
        ca, sa = np.cos(pa[2]), np.sin(pa[2]); d = pb - pa
        return np.array([ca * d[0] + sa * d[1], -sa * d[0] + ca * d[1], mm.mod2pi(d[2])]) + rng.normal(0, 0.02, 3) + np.asarray(off, float)
    zr, zm, zm2 = meas(5, 9, (0.6, -0.4, 0.1)), meas(6, 2), meas(6, 2, (2.0, 1.0, 0.5))
    pts = sc["start"]
    q = pts[7, :2] - pts[5, :2]; c5, s5 = np.cos(pts[5, 2]), np.sin(pts[5, 2])
    qq = np.array([c5 * q[0] + s5 * q[1], -s5 * q[0] + c5 * q[1]])
    zp = np.array([np.hypot(*qq) + 0.03, np.arctan2(qq[1], qq[0]) - 0.02]); Wp = np.array([[900.0, 30.0], [30.0, 2500.0]])
    rg = np.random.default_rng(64)
    xb, et, Lm = gg.random_gaussian(rg, "relative", 2)
    gnat = ([5, 1], pts[[5, 1]] + rg.normal(0, 0.05, (2, 3)), et, Lm)
    xb2, et2, Lm2 = gg.random_gaussian(rg, "regular", 2)
    ghost = ([10, 6], pts[[10, 6]] + rg.normal(0, 0.05, (2, 3)), et2, Lm2)
    remove = [5, 6]

    def make(on_host):
        g = gg.build(lib, sc)
        g.add_factor_xyt(5, 9, zr, W); rb = g.n_factors - 1
        assert g.set_robust(rb, abi.ROBUST_CAUCHY, 1.0) == 0
        mxi = g.add_factor_max(6, 2, [zm, zm2], [W.ravel(), 0.1 * W.ravel()], [0.0, -1.0])
        g.add_factor_polar(abi.POLAR_RANGE_BEARING, 5, 7, zp, Wp)
        g.add_factor_gaussian(*(ghost if on_host else gnat))
        return g, rb, mxi

    for on_host in (0, 1):
        with lib.options(gaussian_on_host=on_host):
            g, rb, mxi = make(on_host); p = lib.new_param()
            g.cholesky(p)
            lp = g.l_points()
            w = g.robust_weights(p, [rb])[0]
            sel = int(g.max_selected(p, [mxi])[0])
            assert 0 < w < 1 and sel in (0, 1)
            ze, We = lib.polar_slot(abi.POLAR_RANGE_BEARING, lp[5], lp[7], zp, Wp)
            eff = dict(start=sc["start"], fa=np.append(sc["fa"], [5, 6, 5]), fb=np.append(sc["fb"], [9, 2, 7]),
                       z=np.vstack([sc["z"], zr, [zm, zm2][sel], ze]), W=np.concatenate([sc["W"], [w * W, [W, 0.1 * W][sel], We]]))
            got = g.marginal_prior(p, remove)
            _check(lib, f"mixed families, gaussian_on_host={on_host}", got, eff, lp, remove, [ghost if on_host else gnat])
            assert len(eff["fa"]) == F0 + 3
            p.destroy(); g.destroy()


def test_forty_nodes_exactly_and_forty_one_refused(lib):
    sc = gg.snake(60, 65, turn=0.1)
    g = gg.build(lib, sc); p = lib.new_param()
    g.cholesky(p)
    lp = g.l_points()
    remove = list(range(10, 48))                                 # 38 removed + 2 blanket nodes
    got = g.marginal_prior(p, remove)
    _check(lib, "|M| + |B| = 40", got, sc, lp, remove)
    lib.clear_error()
    out = _raw(lib, g, p, list(range(10, 49)), 40)
    assert out[0] == -12 and _untouched(out) and "40" in lib.last_error()[1]
    out = _raw(lib, g, p, [20], 1)                               # |B| = 2 > cap
    assert out[0] == -12 and _untouched(out)
    rc, nk, *_ = _raw(lib, g, p, [], 0)                           # m == 0
    assert rc == 0 and nk == 0
    p.destroy(); g.destroy()


# ---- 6. exactness end to end ---------------------------------------------------------------------------------------------------------------
def _snake12():
    return gg.snake(12, 66, closures=[(0, 11), (2, 9), (5, 10)])


def test_reduced_graph_takes_the_full_graph_s_step(lib):
    sc = _snake12()
    remove = [3, 4, 7]
    kept = [i for i in range(12) if i not in remove]
    g = gg.build(lib, sc); p = lib.new_param(); p.c.tikhanov = 0.0
    g.cholesky(p)
    lp, dx_full = g.l_points(), g.deltas().copy()
    cov_full = g.marginals(p, kept)
    g.set_all_states(lp)                                           # every kept node back at the linearisation point
    fi, idx = g.marginalize(p, remove)
    assert list(idx) == [0, 1, 2, -1, -1, 3, 4, -1, 5, 6, 7, 8] and g.n_nodes == 9 and fi == g.n_factors - 1
    k = g.get_gaussian(fi)
    B = [2, 5, 6, 8]                                               # the neighbours of 3, 4 and 7: no closure touches them
    assert k == len(B) and [g.factor(fi).nodes[j] for j in range(k)] == [int(idx[b]) for b in B]
    assert np.array_equal(g.states(), lp[kept])
    g.cholesky(p)
    dx_red = g.deltas()
    cov_red = g.marginals(p, list(range(9)))
    d64 = gg.model_step(sc, lp, [], 0.0)
    dl = gg.model_step(sc, lp, [], 0.0, np.longdouble)
    allowed, own = 10 * _dev(dx_full, dl), _dev(dx_full, dl)
    print(f"marginalize exactness: full graph |device - longdouble| = {own:.3e} (float64 model: {_dev(d64, dl):.3e}); reduced against full "
          f"{_dev(dx_red, dx_full[kept].astype(np.longdouble)):.3e}, allowed {allowed:.3e}")
    assert _dev(dx_red, dx_full[kept].astype(np.longdouble)) <= allowed
    A, _ = gg.model_system(sc, lp, [], 0.0, np.longdouble)
    Sl = mm.solve_spd(A, np.eye(36, dtype=np.longdouble), np.longdouble)
    own_cov = max(_dev(cov_full[j], Sl[3 * i:3 * i + 3, 3 * i:3 * i + 3]) for j, i in enumerate(kept))
    print(f"marginalize exactness: marginals full |device - longdouble| = {own_cov:.3e}, reduced against full {_dev(cov_red, cov_full.astype(np.longdouble)):.3e}")
    assert _dev(cov_red, cov_full.astype(np.longdouble)) <= 10 * own_cov
    p.destroy(); g.destroy()


# ---- 7. optimisers on the reduced graph ------------------------------------------------------------------------------------------------------
def test_lm_gnc_and_the_resident_loop_on_the_reduced_graph(lib):
    sc = _snake12()
    remove = [3, 4, 7]
    g = gg.build(lib, sc); p = lib.new_param()
    r = g.optimize_lm(p, max_iters=60)
    assert r["status"] in (1, 2) and r["accepted"] >= 2
    h_last = float(np.max(np.abs(g.deltas())))                     # delta_X after an LM run: the last accepted step
    assert h_last > 0
    # (an LM run keeps no factorisation -- its last system carries the damping: one batch call at the stop point, whose own step is below
    # LM's last, leaves the linearisation the prior is taken from)
    at_stop = g.states().copy()
    g.cholesky(p)
    assert np.max(np.abs(g.states() - at_stop)) <= h_last
    g.marginalize(p, remove)
    stop = g.states().copy()
    steps_red = []
    for _ in range(4):                                             # single iterations: every accepted step is seen (a rejected one moves nothing)
        before = g.states().copy()
        g.optimize_lm(p, max_iters=1)
        steps_red.append(float(np.max(np.abs(g.states() - before))))
    print(f"LM steps: the full graph's last accepted {h_last:.3e}, the reduced graph's {steps_red}")
    assert max(steps_red) <= h_last, (steps_red, h_last)
    rep = g.optimize_lm(p, max_iters=50)
    assert rep["status"] in (1, 2, 3)
    # from a small perturbation back to the stop point.  Each run stops when a step lowers F by less than ftol F: with F - F* ~ 1/2 e'He the
    # distance to the minimum is then at most sqrt(2 ftol F / lambda_min(H)) -- twice that between two runs
    opt = g.states().copy()
    fi = g.n_factors - 1
    f = g.factor(fi); k = f.nnodes; n = 3 * k
    prior = ([f.nodes[j] for j in range(k)], np.array([f.u.z[j] for j in range(n)]).reshape(k, 3), np.array([f.u.z[n + j] for j in range(n)]),
             np.array(C.cast(C.cast(f.u.W, C.c_void_p).value + 8, C.POINTER(C.c_double * (n * n))).contents).reshape(n, n))
    kept = [i for i in range(12) if i not in remove]
    new = {old: j for j, old in enumerate(kept)}
    keepf = [i for i in range(len(sc["fa"])) if sc["fa"][i] not in remove and sc["fb"][i] not in remove]
    red = dict(start=opt, fa=np.array([new[a] for a in sc["fa"][keepf]]), fb=np.array([new.get(b, -1) for b in sc["fb"][keepf]]), z=sc["z"][keepf], W=sc["W"][keepf])
    H, _ = gg.model_system(red, opt, [prior], 0.0)
    lam_min = float(np.linalg.eigvalsh(H)[0])
    bound = 2 * np.sqrt(2 * 1e-10 * max(rep["F_final"], 1e-300) / lam_min)
    rng = np.random.default_rng(67)
    g.set_all_states(opt + rng.normal(0, 1e-3, opt.shape))
    r = g.optimize_lm(p, max_iters=50)
    assert r["status"] in (1, 2)
    back = float(np.max(np.abs(g.states() - opt)))
    print(f"LM back from a 1e-3 perturbation: {back:.3e} from the stop point, bound {bound:.3e}")
    assert back <= bound
    # the resident loop and GNC (the prior not a candidate) against repeated batch calls, from the same start
    start = stop + rng.normal(0, 0.02, stop.shape)
    g.set_all_states(start)
    for _ in range(4):
        g.cholesky(p)
    batch = g.states().copy()
    g.set_all_states(start)
    g.batch_resident(p, 4)
    assert np.max(np.abs(g.states() - batch)) < 1e-11
    g.set_all_states(start)
    cand = [i for i in range(g.n_factors - 1) if g.factor(i).nnodes == 2][-2:]
    r = g.optimize_gnc(p, cand, c=1000.0, max_stages=4, max_iters=30)
    assert np.all(r["weights"] > 0.999) and np.max(np.abs(g.states() - batch)) < 1e-4
    p.destroy(); g.destroy()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused(lib, g, p, remove, code, word, cap=40):
    before = (g.states().copy(), g.l_points().copy(), g.n_nodes, g.n_factors, [C.addressof(g.factor(i)) for i in range(g.n_factors)])
    lib.clear_error()
    out = _raw(lib, g, p, remove, cap)
    c, msg = lib.last_error()
    assert out[0] == code == c and word in msg and _untouched(out), (out[0], c, msg)
    lib.clear_error()
    idx = np.full(g.n_nodes, -7, np.int32)
    rm = np.ascontiguousarray(remove, np.int32)
    rc = lib.dll.aprilsam_amd_graph_marginalize(g.ptr, p.ptr, len(rm), rm.ctypes.data_as(_ip), idx.ctypes.data_as(_ip))
    assert rc == code and lib.last_error()[0] == code and (idx == -7).all()
    after = (g.states(), g.l_points(), g.n_nodes, g.n_factors, [C.addressof(g.factor(i)) for i in range(g.n_factors)])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    return msg


def test_refusals(lib):
    sc = _snake12()
    rng = np.random.default_rng(68)
    g = gg.build(lib, sc); p = lib.new_param()
    _refused(lib, g, p, [3], -1, "no retained factor")                      # no solve yet
    g.cholesky(p)
    _refused(lib, g, p, [12], -13, "out of range")
    _refused(lib, g, p, [3, 3], -13, "twice")
    q = lib.new_param()
    g.cholesky(q)                                                           # another param stepped the graph: p's linearisation is stale
    _refused(lib, g, p, [3], -1, "another")
    g.cholesky(p)
    assert g.set_fixed(2) == 0
    g.cholesky(p)
    _refused(lib, g, p, [3], -12, "fixed")                                  # node 2 is in the blanket of 3
    _refused(lib, g, p, [2], -12, "fixed")
    assert g.set_fixed(2, False) == 0
    tri = g.add_factor_gaussian([1, 6, 10], sc["start"][[1, 6, 10]], np.zeros(9), gg.random_gaussian(rng, "relative", 3)[2])
    g.cholesky(p)
    msg = _refused(lib, g, p, [6], -12, "more than two nodes")              # a 3-node factor touching M
    assert str(tri) in msg
    assert len(g.marginal_prior(p, [4])[0]) == 2                            # ... elsewhere the same graph is fine
    p.destroy(); q.destroy(); g.destroy()


def test_blanket_of_twelve_is_refused_by_marginalize_only(lib):
    n = 14
    sc = gg.snake(n, 69, closures=[(0, j) for j in range(2, 13)])           # a star of closures on pose 0: 12 neighbours
    g = gg.build(lib, sc); p = lib.new_param()
    g.cholesky(p)
    keep = g.marginal_prior(p, [0])[0]
    assert len(keep) == 12
    before = (g.n_nodes, g.n_factors, g.states().copy())
    lib.clear_error()
    rm = np.array([0], np.int32)
    rc = lib.dll.aprilsam_amd_graph_marginalize(g.ptr, p.ptr, 1, rm.ctypes.data_as(_ip), None)
    code, msg = lib.last_error()
    assert rc == code == -12 and "12" in msg and "aprilsam_amd_graph_marginalize" in msg
    assert (g.n_nodes, g.n_factors) == before[:2] and np.array_equal(g.states(), before[2])
    g.cholesky(p)                                                           # the param kept its plan and the graph its device copy
    assert p.stats()["not_spd"] == 0
    p.destroy(); g.destroy()


def test_removed_block_that_is_not_positive_definite(lib):
    """M is a free-floating component: two poses tied to each other and to nothing else, headings 0, z = 0, W = I, so H_MM =
    [[I, -I], [-I, I]] in exact arithmetic.  At tikhanov = 0 the solver call itself reports the system (-2) and keeps no factor: the prior
    is unavailable (-1).  With the tikhanov term the call succeeds and the factor is kept; the removed block, taken from the slots alone
    (no lambda), is singular: -2 from the prior, nothing written, the param keeps its factorisation."""
    sc = gg.snake(6, 70)
    g = gg.build(lib, sc)
    a = g.add_node_xyt([10.0, 10.0, 0.0]); b = g.add_node_xyt([10.0, 10.0, 0.0])
    g.add_factor_xyt(a, b, [0.0, 0.0, 0.0], np.eye(3))
    p = lib.new_param(); p.c.tikhanov = 0.0
    g.cholesky(p)
    assert p.stats()["not_spd"] == 1
    _refused(lib, g, p, [a, b], -1, "no retained factor")
    p.c.tikhanov = LAM
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    _refused(lib, g, p, [a, b], -2, "not positive")
    assert len(g.marginal_prior(p, [2])[0]) == 2                             # the param kept its factorisation
    # a component removed whole with a regular block: B is empty, nothing but n_keep is written
    h = gg.build(lib, sc)
    c = h.add_node_xyt([10.0, 10.0, 0.0]); h.add_factor_xytpos(c, [10.0, 10.0, 0.0], np.eye(3))
    hp = lib.new_param()
    h.cholesky(hp)
    rc, nk, keep, xbar, eta, L = _raw(lib, h, hp, [c], 4)
    assert rc == 0 and nk == 0 and (keep == -7).all() and np.isnan(xbar).all() and np.isnan(eta).all() and np.isnan(L).all()
    fi, idx = h.marginalize(hp, [c])
    assert fi is None and h.n_nodes == 6 and h.n_factors == len(sc["fa"]) and list(idx) == [0, 1, 2, 3, 4, 5, -1]
    h.cholesky(hp)
    assert hp.stats()["not_spd"] == 0
    for x in (p, hp):
        x.destroy()
    g.destroy(); h.destroy()
