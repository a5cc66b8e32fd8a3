"""aprilsam_amd_optimize_gnc on the GPU: parity with the numpy model (tests/support/gnc_model.py) on the snake
scenarios, every kernel path, determinism, what the call is for, the contract it leaves behind, and every refusal."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import abi
from aprilsam_amd.host import GncError, MarginalsError
from tests.support import gnc_model as G
from tests.support import lm_model, robust_model
from tests.support.kernel_paths import KERNEL_PATHS

pytestmark = pytest.mark.gpu

LOSSES = [G.GM, G.TLS]
LOSS_IDS = ["GM", "TLS"]
CC = G.C_DEFAULT ** 2


def _graph(lib, x, plain):
    g = lib.new_graph(); g.build_from_arrays(x, *plain)
    return g


def _ang(a, b):
    d = a - b
    d[:, 2] = lm_model.mod2pi(d[:, 2])
    return np.abs(d).max()


def _run(lib, sc, loss, **kw):
    g = _graph(lib, sc["start"], sc["plain"]); p = lib.new_param()
    r = g.optimize_gnc(p, sc["cand"], trace=True, loss=loss, **kw)
    return r, g, p


def _schedule(loss, mu0, n, step=1.4):
    mus = [mu0]
    for _ in range(n - 1):
        mus.append(max(1.0, mus[-1] / step) if loss == G.GM else mus[-1] * step)
    return np.array(mus)


def _same_as_the_model(r, x, sc, ref, loss, name=""):
    """the tolerances of tests/test_gpu_lm.py, for its reasons: one evaluation at 1e-12, F and the states (solves) at 1e-9, decisions
    exact outside lm_model.comparable_rows' band"""
    assert abs(r["s_max"] - ref["s_max"]) <= 1e-12 * ref["s_max"], name
    assert abs(r["mu_initial"] - ref["mu_initial"]) <= 1e-12 * ref["mu_initial"], name
    assert r["mu_initial"] == G.mu_start(loss, G.C_DEFAULT, r["s_max"])[0]
    assert (r["status"], r["stages"]) == (ref["status"], ref["stages"]), (name, r["status"], r["stages"], ref["stages"])
    t, rt = r["stage_trace"], ref["stage_trace"]
    assert t.shape == rt.shape
    # the schedule: exactly the rule applied to the device's own mu_0 (which the model's matches to rounding)
    assert np.array_equal(t[:, 0], _schedule(loss, r["mu_initial"], r["stages"])), name
    assert np.all(np.abs(t[:, 0] - rt[:, 0]) <= 1e-12 * rt[:, 0]) and r["mu_final"] == t[-1, 0]
    dF = np.abs(t[:, 1:3] - rt[:, 1:3]) / np.abs(rt[:, 1:3])
    print(name, "per-stage F: max relative difference", dF.max(), "iterations", r["iterations"], ref["iterations"])
    assert np.all(dF <= 1e-9), (name, dF.max())
    for k, (F0, lt) in enumerate(ref["lm_traces"]):
        if lm_model.comparable_rows(lt, F0) == len(lt):          # (the whole stage lies outside the round-off band)
            assert t[k, 3] == len(lt), (name, k, t[k, 3], len(lt))
    assert r["iterations"] == int(t[:, 3].sum()) and abs(r["F_final"] - ref["F_final"]) <= 1e-9 * ref["F_final"]
    assert _ang(x.copy(), ref["x"]) < 1e-9, (name, _ang(x.copy(), ref["x"]))
    s = robust_model.s_of(x, sc["plain"])[sc["cand"]]
    assert np.array_equal(s <= CC, ref["s"] <= CC) and r["n_inliers"] == ref["n_inliers"]
    assert not (s <= CC)[sc["is_false"]].any() and (s <= CC)[~sc["is_false"]].all()
    w = G.weight(loss, G.C_DEFAULT, r["mu_final"], s)
    assert np.all(np.abs(r["weights"] - w) <= 1e-12 * np.maximum(np.abs(w), 1e-300)), (name, np.abs(r["weights"] - w).max())
    assert abs(r["F_final"] - G.cost(x, sc["plain"], sc["cand"], loss, G.C_DEFAULT, r["mu_final"])) <= 1e-12 * r["F_final"]
    assert abs(r["chi2_final"] - robust_model.chi2(x, sc["plain"], 0, 1.0)) <= 1e-12 * r["chi2_final"]


@pytest.mark.parametrize("case", G.CASES, ids=str)
@pytest.mark.parametrize("loss", LOSSES, ids=LOSS_IDS)
def test_parity_with_the_model(lib, case, loss):
    sc = G.snake(*case)
    r, g, p = _run(lib, sc, loss)
    _same_as_the_model(r, g.states(), sc, G.model_run(case, loss), loss, f"{case} {loss}")
    assert g.states().tobytes() == g.l_points().tobytes()
    p.destroy(); g.destroy()


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items())


@pytest.mark.parametrize("opts", KERNEL_PATHS + [dict(tagged_x=0), dict(tagged_x=1), dict(tagged_x=2)], ids=_ids)
def test_every_kernel_path(lib, opts):
    case = (6, 6, 3)
    sc = G.snake(*case)
    with lib.options(**opts):
        r, g, p = _run(lib, sc, G.GM)
        _same_as_the_model(r, g.states(), sc, G.model_run(case, G.GM), G.GM, _ids(opts))
        p.destroy(); g.destroy()


@pytest.mark.parametrize("loss", LOSSES, ids=LOSS_IDS)
def test_determinism_and_check_every(lib, loss):
    sc = G.snake(6, 6, 3)
    out = []
    for ce in (1, 1, 7):
        r, g, p = _run(lib, sc, loss, check_every=ce)
        out.append((r, g.states().tobytes(), g.deltas().tobytes()))
        p.destroy(); g.destroy()
    r0 = out[0][0]
    for r, s, d in out[1:]:
        assert s == out[0][1] and d == out[0][2]
        assert r["stage_trace"].tobytes() == r0["stage_trace"].tobytes() and r["weights"].tobytes() == r0["weights"].tobytes()
        assert {k: v for k, v in r.items() if k not in ("stage_trace", "weights")} == {k: v for k, v in r0.items() if k not in ("stage_trace", "weights")}


def test_it_does_what_it_is_for(lib):
    """From the dead-reckoned start of (6, 10, 5) plain LM ends metres off and GNC within 0.1 of the truth.  Cauchy on every closure: the
    model (tests/support/robust_model.py) DOES reject all ten false closures from this start and ends 0.0979 off -- between GNC-GM
    (0.0996) and GNC-TLS (0.0960).  The statement the model supports is the one kept: Cauchy ends with a larger error than GNC with TLS,
    whose inliers keep weight exactly 1 where Cauchy down-weights every closure it keeps."""
    sc = G.snake(6, 10, 5)
    g = _graph(lib, sc["start"], sc["plain"]); p = lib.new_param()
    g.optimize_lm(p)
    e_lm = G.position_error(g.states(), sc["truth"])
    p.destroy(); g.destroy()
    g = _graph(lib, sc["start"], sc["plain"]); p = lib.new_param()
    for i in sc["cand"]:
        assert g.set_robust(int(i), abi.ROBUST_CAUCHY, G.C_DEFAULT) == 0
    g.optimize_lm(p, max_iters=50)
    e_cauchy = G.position_error(g.states(), sc["truth"])
    p.destroy(); g.destroy()
    e = {}
    for loss in LOSSES:
        r, g, p = _run(lib, sc, loss)
        e[loss] = G.position_error(g.states(), sc["truth"])
        assert r["status"] == 1 and r["n_inliers"] == int((~sc["is_false"]).sum())
        p.destroy(); g.destroy()
    print("position error: LM", e_lm, "Cauchy", e_cauchy, "GNC-GM", e[G.GM], "GNC-TLS", e[G.TLS])
    assert e_lm > 1.0
    assert e[G.GM] < 0.1 and e[G.TLS] < 0.1
    assert e_cauchy > e[G.TLS]


def test_contract(lib):
    case = (6, 6, 3)
    sc = G.snake(*case)
    x0, plain, cand = sc["start"], sc["plain"], sc["cand"]
    g = _graph(lib, x0, plain); p = lib.new_param()
    p.c.tikhanov = 3e-4
    gr = _graph(lib, x0, plain); pr = lib.new_param(); pr.c.tikhanov = 3e-4
    gr.cholesky(pr)                                 # (a param with the plan of the same start that never runs GNC)
    dx_before = g.deltas().copy()
    r = g.optimize_gnc(p, cand, trace=True)
    xs = g.states()
    assert r["status"] == 1 and xs.tobytes() == g.l_points().tobytes()
    assert not np.isnan(g.deltas()).any() and g.deltas().tobytes() != dx_before.tobytes()
    assert p.c.tikhanov == 3e-4
    assert all(g.get_robust(int(i)) == (abi.ROBUST_NONE, 0.0) for i in cand)
    assert np.all(g.robust_weights(p, cand) == -1.0)
    with pytest.raises(MarginalsError) as e:
        g.marginals(p)
    assert e.value.code == -1
    # The plain step after the call gives the bits it gives on a fresh graph built at the returned states.  A plan takes a hint from the
    # nodes' coordinates (another start: another elimination order, other rounding -- tests/test_gpu_lm.py meets the same), so each
    # comparison is between params planned from the same states: the graph (its factor objects, its packed W slots) with a new param
    # against the fresh graph with a new param, then the param that ran GNC against one planned from the same start that never did
    gf = _graph(lib, xs, plain); pf = lib.new_param(); pf.c.tikhanov = 3e-4
    c_g, c_f = g.chi2(), gf.chi2()
    assert c_g == c_f and abs(c_g - r["chi2_final"]) <= 1e-12 * c_g
    p2 = lib.new_param(); p2.c.tikhanov = 3e-4
    g.cholesky(p2); gf.cholesky(pf)
    assert g.states().tobytes() == gf.states().tobytes() and g.deltas().tobytes() == gf.deltas().tobytes()
    assert g.marginals(p2).tobytes() == gf.marginals(pf).tobytes()
    p2.destroy()
    g.set_all_states(xs, relinearize=True); g.cholesky(p)
    gr.set_all_states(xs, relinearize=True); gr.cholesky(pr)
    assert g.states().tobytes() == gr.states().tobytes() and g.deltas().tobytes() == gr.deltas().tobytes()
    assert np.abs(g.states() - gf.states()).max() < 1e-12
    assert g.marginals(p).tobytes() == gr.marginals(pr).tobytes()
    # plain LM on the param after GNC: the bits of a param that never ran it
    g.set_all_states(x0, relinearize=True); gr.set_all_states(x0, relinearize=True)
    a = g.optimize_lm(p, trace=True); b = gr.optimize_lm(pr, trace=True)
    assert a["trace"].tobytes() == b["trace"].tobytes() and g.states().tobytes() == gr.states().tobytes()
    for o in (p, g, pr, gr, pf, gf):
        o.destroy()


def test_one_captured_graph_serves_every_stage(lib):
    sc = G.snake(6, 6, 3)
    full = G.model_run((6, 6, 3), G.TLS)["stages"]
    assert full > 5
    counts = {}
    for stages in (2, 5, 100):
        r, g, p = _run(lib, sc, G.TLS, max_stages=stages)
        assert r["stages"] == min(stages, full) and r["status"] == (2 if stages < full else 1)
        counts[stages] = p.graph_captures()
        p.destroy(); g.destroy()
    assert counts[2] == counts[5] == counts[100] and 1 <= counts[2] <= 2, counts
    with lib.options(use_graph=0):
        r, g, p = _run(lib, sc, G.TLS, max_stages=5)
        assert p.graph_captures() == 0
        p.destroy(); g.destroy()


def test_non_candidates_keep_their_own_behaviour(lib):
    """A robust factor and a max factor among the non-candidates.  From a start where every candidate is an inlier TLS runs ONE stage with
    all weights 1 and rho = s: the run must be optimize_lm's with the same options on the same graph, bit for bit -- and on the way the
    robust factor was weighted and the max factor selected as there."""
    sc = G.snake(6, 0, 3)
    plain, cand = sc["plain"], sc["cand"]
    x0 = lm_model.optimize(sc["start"], plain)["x"]
    x0[:, :2] += np.random.default_rng(1).normal(0.0, 0.01, (len(x0), 2))
    rb, others = int(cand[0]), cand[1:]
    W = np.asarray(plain[3][0], float)

    def build():
        g = _graph(lib, x0, plain)
        assert g.set_robust(rb, abi.ROBUST_HUBER, 0.5) == 0
        m = g.add_factor_max(3, 20, [G._measure(sc["truth"][3], sc["truth"][20]), [0.0, 0.0, 0.0]], [W, 1e-6 * W], [0.0, -2.0])
        return g, m

    g, m = build(); p = lib.new_param()
    r = g.optimize_gnc(p, others, trace=True, loss=G.TLS)
    assert r["status"] == 1 and r["stages"] == 1 and np.isinf(r["mu_initial"]) and np.all(r["weights"] == 1.0) and r["n_inliers"] == len(others)
    g2, _ = build(); p2 = lib.new_param()
    r2 = g2.optimize_lm(p2, trace=True, max_iters=10)
    assert r["iterations"] == r2["iterations"] and r["accepted"] == r2["accepted"] and r2["iterations"] >= 2
    assert r["F_final"] == r2["F_final"] and r["chi2_final"] == r2["chi2_final"]
    assert np.array_equal(r["stage_trace"][0], [np.inf, r2["F_initial"], r2["F_final"], r2["iterations"]])
    assert g.states().tobytes() == g2.states().tobytes() and g.deltas().tobytes() == g2.deltas().tobytes()
    assert g.robust_weights(p, [rb])[0] == g2.robust_weights(p2, [rb])[0] and 0 < g.robust_weights(p, [rb])[0] <= 1
    assert g.max_selected(p, [m])[0] == g2.max_selected(p2, [m])[0] == 0
    for o in (p, g, p2, g2):
        o.destroy()


def _expect(fn, code):
    with pytest.raises(GncError) as e:
        fn()
    assert e.value.code == code, e.value.code


def test_every_refusal_leaves_the_graph_and_param_usable(lib, tmp_path):
    from tests.support import custom_scenario
    from tests.support.asym_scenarios import batch_graph
    case = (4, 3, 3)
    sc = G.snake(*case)
    x0, plain, cand = sc["start"], sc["plain"], sc["cand"]
    ref = G.model_run(case, G.GM)

    def check(g, p, code, cand=cand, **kw):
        s, l, d = g.states().copy(), g.l_points().copy(), g.deltas().copy()
        _expect(lambda: g.optimize_gnc(p, cand, **kw), code)
        assert lib.last_error()[0] == code
        assert s.tobytes() == g.states().tobytes() and l.tobytes() == g.l_points().tobytes() and d.tobytes() == g.deltas().tobytes()

    def good(g, p, cand=cand):
        r = g.optimize_gnc(p, cand, trace=True)
        _same_as_the_model(r, g.states(), sc, ref, G.GM)

    # bad options and candidate lists
    g = _graph(lib, x0, plain); p = lib.new_param()
    for bad in (dict(loss=0), dict(c=-1.0), dict(mu_step=1.0), dict(max_stages=0), dict(max_iters=0), dict(check_every=0), dict(lambda0=-1.0)):
        check(g, p, -13, **bad)
    for bad in ([], None, [int(cand[0]), g.n_factors], [-1], [int(cand[0]), int(cand[0])]):
        check(g, p, -13, cand=bad)
    # candidates that cannot carry the surrogate: a loss of its own, W not positive definite, a max factor (appended last: the rest of
    # the graph stays the model's once the loss is cleared and the appended factors' weights vanish ...)
    assert g.set_robust(int(cand[1]), abi.ROBUST_DCS, 2.0) == 0
    check(g, p, -12)
    assert g.set_robust(int(cand[1]), abi.ROBUST_NONE) == 0
    good(g, p)
    gm = _graph(lib, x0, plain); pm = lib.new_param()
    W = np.asarray(plain[3][0], float)
    m = gm.add_factor_max(0, 5, [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [W, W], [0.0, -1.0])
    check(gm, pm, -12, cand=[int(cand[0]), m])
    gm.add_factor_xyt(0, 7, [1.0, 0.0, 0.0], np.diag([1.0, -1.0, 1.0]).reshape(9))
    check(gm, pm, -12, cand=[gm.n_factors - 1])
    assert gm.optimize_gnc(pm, cand)["status"] in (1, 2)
    # empty graph
    ge = lib.new_graph()
    check(ge, p, -1, cand=[0])
    # host-evaluated factor
    cl = custom_scenario.build_custom_lib(str(tmp_path))
    gh = _graph(lib, x0, plain); ph = lib.new_param()
    lib._add_factor(gh.ptr, cl.custom_heading_create(3, 0.2, 5.0))
    check(gh, ph, -4)
    check(gh, ph, -12, cand=[gh.n_factors - 1])
    gh.cholesky(ph)
    assert ph.stats()["error_code"] == 0
    # asymmetric information matrix anywhere
    arr = batch_graph()
    ga = _graph(lib, arr[0], arr[1:]); pa = lib.new_param()
    check(ga, pa, -12, cand=[int(np.nonzero(np.asarray(arr[2]) >= 0)[0][0])])
    ga.cholesky(pa)
    assert pa.stats()["error_code"] == 0
    # sharded param
    d = lib.dll
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    d.aprilsam_amd_shard_end.argtypes = [C.c_void_p]
    gs = _graph(lib, x0, plain); ps = lib.new_param()
    assert d.aprilsam_amd_shard_begin(C.cast(gs.ptr, C.c_void_p), C.cast(ps.ptr, C.c_void_p), 0, 1) == 0
    check(gs, ps, -12)
    d.aprilsam_amd_shard_end(C.cast(ps.ptr, C.c_void_p))
    good(gs, ps)
    for o in (p, g, pm, gm, ge, ph, gh, pa, ga, ps, gs):
        o.destroy()
