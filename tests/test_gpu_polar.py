"""Range / bearing / range-bearing factors on the GPU: batch steps, LM, the resident loop, every kernel path,
incremental runs and the consumers of the retained factor against the numpy model of the true m-row factors
(tests/support/polar_model.py) and against the same graphs with the polar factors evaluated on the host through their own eval()
(debug option polar_on_host); every refusal.  Tolerance: the project's 1e-9, relative to the largest entry compared."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import abi, datasets, host
from tests.support import lm_model
from tests.support import polar_model as pm
from tests.support.kernel_paths import KERNEL_PATHS
from tests.support.normal_eq import mod2pi

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(f"{what}: deviation {err:.3e}")
    assert err <= tol, (what, err)
    return err


def _states_close(got, want, what, tol=TOL):
    d = np.asarray(got) - np.asarray(want)
    d[:, 2] = mod2pi(d[:, 2])
    return _close(d, np.zeros_like(d), what, tol * max(1.0, np.abs(want[:, :2]).max()))


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _resident(lib, g, p, steps):
    d = lib.dll
    assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, steps, 0) == 0
    assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
    chi = d.aprilsam_amd_resident_chi2(g.ptr)
    assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    return chi


@pytest.fixture(scope="module")
def small():
    """6 poses + 3 landmarks, all three kinds"""
    d = pm.snake(3, 3, seed=7, n_rows=2)
    assert {p[0] for p in d["polars"]} == {pm.RANGE, pm.BEARING, pm.RANGE_BEARING} and d["n_poses"] == 6
    return d


@pytest.fixture(scope="module")
def medium():
    """K = 6, L = 8"""
    return pm.snake(6, 8, seed=2)


# ---- 1. one batch step ---------------------------------------------------------------------------------------------------------
def test_one_batch_step_against_the_model(lib, small):
    d = small
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    assert p.c.tikhanov == pm.TIKHANOV
    _close(g.chi2(), pm.chi2(d["start"], d["plain"], d["polars"]), "chi2 at the start")
    lib.clear_error()
    g.cholesky(p)
    dx, x1 = pm.gn_step(d["start"], d["plain"], d["polars"], pm.TIKHANOV)
    assert p.stats()["not_spd"] == 0 and lib.last_error()[0] == 0
    _close(g.deltas(), dx, "dx")
    _states_close(g.states(), x1, "states")
    assert np.array_equal(g.l_points(), d["start"])
    _close(g.chi2(), pm.chi2(x1, d["plain"], d["polars"]), "chi2 after the step")
    p.destroy(); g.destroy()


# ---- 2. degenerate start ---------------------------------------------------------------------------------------------------
def test_landmark_on_its_observer_is_silent_for_the_step(lib, small):
    d = small
    k = next(i for i, pol in enumerate(d["polars"]) if pol[0] == pm.RANGE_BEARING)
    kind, a, b, _, _ = d["polars"][k]
    x0 = d["start"].copy()
    x0[b, :2] = x0[a, :2]                      # rho^2 == 0 for EVERY factor between a and b; the others still see the landmark
    silent = [i for i, pol in enumerate(d["polars"]) if (pol[1], pol[2]) == (a, b)]
    rest = [pol for i, pol in enumerate(d["polars"]) if i not in silent]
    assert any(pol[2] == b for pol in rest)
    g = pm.build(lib, x0, d["plain"], d["polars"]); p = lib.new_param()
    lib.clear_error()
    g.cholesky(p)
    assert lib.last_error()[0] == 0 and p.stats()["not_spd"] == 0
    assert np.all(np.isfinite(g.states())) and np.all(np.isfinite(g.deltas()))
    dx, x1 = pm.gn_step(x0, d["plain"], rest, pm.TIKHANOV)
    _close(g.deltas(), dx, "dx without the silent factor")
    _states_close(g.states(), x1, "states without the silent factor")
    _close(g.chi2(), pm.chi2(x1, d["plain"], d["polars"]), "chi2 (the factor counts again away from the point)")
    p.destroy(); g.destroy()


def test_edit_in_place_is_seen_by_the_next_call(lib, small):
    """z and W of a packed polar factor edited in place between two calls (the reference re-reads every factor on every call): the warm
    call, the resident loop and chi2 use the edited values -- the bits of a fresh graph built with them"""
    d = small
    k = next(i for i, pol in enumerate(d["polars"]) if pol[0] == pm.RANGE_BEARING)
    kind, a, b, zz, WW = d["polars"][k]
    z2, W2 = zz + [0.05, -0.02], WW * 1.5
    edited = list(d["polars"]); edited[k] = (kind, a, b, z2, W2)
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    g.cholesky(p); g.cholesky(p)                # (cold, then warm: the plan and the captured graph exist)
    x = g.states()
    f = g.factor(len(d["plain"][0]) + k)
    Wd = C.cast(C.cast(f.u.W, C.c_void_p).value + 8, C.POINTER(C.c_double))
    for i in range(2):
        f.u.z[i] = z2[i]
    for i in range(4):
        Wd[i] = W2.ravel()[i]
    gf = pm.build(lib, x, d["plain"], edited); pf = lib.new_param()
    assert g.chi2() == gf.chi2()
    g.cholesky(p); gf.cholesky(pf)
    assert g.states().tobytes() == gf.states().tobytes() and g.chi2() == gf.chi2()
    _states_close(g.states(), pm.gn_step(x, d["plain"], edited, pm.TIKHANOV)[1], "states after the edit against the model")
    for gg, pp in ((g, p), (gf, pf)):
        pp.destroy(); gg.destroy()


# ---- 3. native against host-evaluated ----------------------------------------------------------------------------------------
def _three_calls(lib, d):
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    out = []
    for _ in range(3):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
        out.append((g.states(), g.chi2()))
    n_host = sum(1 for i in range(g.n_factors) if g.get_polar(i))
    p.destroy(); g.destroy()
    return out, n_host


def test_native_against_host_evaluated(lib, medium):
    native, n_polar = _three_calls(lib, medium)
    again, _ = _three_calls(lib, medium)
    with lib.options(polar_on_host=1):
        hosted, _ = _three_calls(lib, medium)
    assert n_polar == len(medium["polars"]) > 20
    x = medium["start"]
    for k in range(3):
        assert native[k][0].tobytes() == again[k][0].tobytes() and native[k][1] == again[k][1]      # two native runs: identical bits
        _states_close(native[k][0], hosted[k][0], f"call {k}: states, native against host-evaluated")
        _close(native[k][1], hosted[k][1], f"call {k}: chi2, native against host-evaluated")
        _, x = pm.gn_step(x, medium["plain"], medium["polars"], pm.TIKHANOV)
        _states_close(native[k][0], x, f"call {k}: states against the model")
        _close(native[k][1], pm.chi2(x, medium["plain"], medium["polars"]), f"call {k}: chi2 against the model")


# ---- 4. LM ---------------------------------------------------------------------------------------------------------------------
_lm_ref = {}


def _lm_model(d, iters):
    if "r" not in _lm_ref:
        _lm_ref["r"] = pm.optimize(d["start"], d["plain"], d["polars"], max_iters=iters)
    return _lm_ref["r"]


def _lm_against_model(lib, d, **opts):
    iters = 25
    ref = _lm_model(d, iters)
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    r = g.optimize_lm(p, trace=True, max_iters=iters, **opts)
    _close(r["F_initial"], ref["F_initial"], "F at the start", 1e-12)
    t, rt = r["trace"], ref["trace"]
    n = lm_model.comparable_rows(rt, ref["F_initial"])
    assert n >= 3
    assert np.array_equal(t[:n, 3], rt[:n, 3])                                   # decisions
    if n == len(rt):
        assert r["iterations"] == ref["iterations"] and r["status"] == ref["status"]
    for k in range(n):
        _close(t[k, 0], rt[k, 0], f"F of iteration {k}")
    _states_close(g.states(), ref["x"], "final states")
    _close(r["chi2_final"], pm.chi2(g.states(), d["plain"], d["polars"]), "chi2_final")
    assert r["F_final"] < 1e-2 * r["F_initial"]
    out = (t.copy(), g.states())
    p.destroy(); g.destroy()
    return out


def test_lm_from_a_dead_reckoned_start(lib, medium):
    a = _lm_against_model(lib, medium)
    b = _lm_against_model(lib, medium)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_lm_without_graph_replay_and_with_sparse_checks(lib, medium):
    base = _lm_against_model(lib, medium)
    with lib.options(use_graph=0):
        o = _lm_against_model(lib, medium, check_every=7)
    # the kernels and their order are the default run's; the host looking less often never changes a result
    n = min(len(o[0]), len(base[0]))
    assert o[0][:n].tobytes() == base[0][:n].tobytes()


def test_gnc_with_xyt_candidates_beside_polar_factors(lib):
    """aprilsam_amd_optimize_gnc, the xyt closures as candidates, on a graph that also holds range-bearing factors to landmarks: the
    schedule, every stage's F and the result are the model's (tests/support/polar_model.py: gnc_optimize)"""
    from tests.support import gnc_model as gm
    sc = gm.snake(6, 3, 1)
    truth, start, polars = pm.with_landmarks(sc["truth"], sc["start"], 6, seed=1)
    ref = pm.gnc_optimize(start, sc["plain"], polars, sc["cand"], gm.TLS)
    g = pm.build(lib, start, sc["plain"], polars); p = lib.new_param()
    r = g.optimize_gnc(p, sc["cand"], trace=True, loss=abi.GNC_TLS)
    _close(r["s_max"], ref["s_max"], "s_max", 1e-12)
    assert (r["status"], r["stages"]) == (ref["status"], ref["stages"]), (r["status"], r["stages"], ref["stages"])
    t, rt = r["stage_trace"], ref["stage_trace"]
    _close(t[:, 0] / rt[:, 0], np.ones(len(rt)), "mu per stage", 1e-12)
    _close(t[:, 1] / rt[:, 1], np.ones(len(rt)), "F on entry per stage")
    _close(t[:, 2] / rt[:, 2], np.ones(len(rt)), "F at the end per stage")
    _states_close(g.states(), ref["x"], "final states")
    _close(r["weights"], ref["weights"], "weights", 1e-12)
    false = np.asarray(sc["is_false"], bool)
    assert np.all(r["weights"][false] == 0.0) and np.all(r["weights"][~false] == 1.0)
    _close(r["chi2_final"], pm.chi2(g.states(), sc["plain"], polars), "chi2_final")
    p.destroy(); g.destroy()


# ---- 5. resident loop ------------------------------------------------------------------------------------------------------------
def test_resident_loop_equals_api_calls(lib, medium):
    d = medium
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    for _ in range(3):
        g.cholesky(p)
    want, chi_want = g.states(), g.chi2()
    gr = pm.build(lib, d["start"], d["plain"], d["polars"]); pr = lib.new_param()
    assert lib.dll.aprilsam_amd_resident_begin(gr.ptr, pr.ptr) == 0               # (no longer -4)
    assert lib.dll.aprilsam_amd_resident_end(gr.ptr, pr.ptr) == 0
    chi = _resident(lib, gr, pr, 3)
    assert np.array_equal(gr.states(), want) and chi == chi_want
    # the same graph with its polar factors on the host: the loop refuses it as it refuses every foreign factor
    with lib.options(polar_on_host=1):
        gh = pm.build(lib, d["start"], d["plain"], d["polars"]); ph = lib.new_param()
        assert lib.dll.aprilsam_amd_resident_begin(gh.ptr, ph.ptr) == -4
        ph.destroy(); gh.destroy()
    for gg, pp in ((g, p), (gr, pr)):
        pp.destroy(); gg.destroy()


# ---- 6. kernel paths ---------------------------------------------------------------------------------------------------------
def _landmark_graph():
    """the 700-pose random graph + range-bearing factors from 120 poses to 20 landmarks"""
    states, fa, fb, z, W = datasets.random_pose_graph(700, 600, 21)
    rng = np.random.default_rng(5)
    N, L = len(states), 20
    lm_xy = states[rng.choice(N, L, replace=False), :2] + rng.normal(0, 1.5, (L, 2))
    x = np.vstack([states, np.column_stack([lm_xy, np.zeros(L)])])
    polars = []
    for l in range(L):
        near = np.argsort(np.hypot(*(states[:, :2] - lm_xy[l]).T))[:6]
        for i in near:
            q = pm.rel(x[i], x[N + l])[0]
            zz = pm.h(pm.RANGE_BEARING, q) + rng.normal(0, [0.05, 0.02])
            polars.append((pm.RANGE_BEARING, int(i), N + l, zz, np.diag([400.0, 2500.0])))
    return x, (np.asarray(fa, np.int64), np.asarray(fb, np.int64), z, W), polars


@pytest.fixture(scope="module")
def landmark_case(lib):
    x, plain, polars = _landmark_graph()
    x2 = pm.gn_steps(x, plain, polars, 2, pm.TIKHANOV)
    return x, plain, polars, x2, _two_steps(lib, x, plain, polars)


def _two_steps(lib, x, plain, polars):
    g = pm.build(lib, x, plain, polars); p = lib.new_param()
    g.cholesky(p); g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    st = g.states()
    p.destroy(); g.destroy()
    return st


@pytest.mark.parametrize("opts", KERNEL_PATHS + [dict(pool_guard=64), dict(pool_poison=1)], ids=_ids)
def test_every_kernel_path(lib, landmark_case, opts):
    x, plain, polars, model, default = landmark_case
    with lib.options(**opts):
        st = _two_steps(lib, x, plain, polars)
    _states_close(st, model, f"{_ids(opts)}: states against the model")
    if opts in (dict(pool_guard=64), dict(pool_poison=1)):
        assert st.tobytes() == default.tobytes()


def test_default_path_against_the_model(lib, landmark_case):
    _states_close(landmark_case[4], landmark_case[3], "default path: states against the model")


# ---- 7. incremental run ----------------------------------------------------------------------------------------------------------
def _compose(pa, z):
    c, s = np.cos(pa[2]), np.sin(pa[2])
    return np.array([pa[0] + c * z[0] - s * z[1], pa[1] + s * z[0] + c * z[1], mod2pi(pa[2] + z[2])])


def _grow(lib, d, steps):
    """the snake grown through april_graph_cholesky_inc: one call after every pose's odometry and one after every polar factor (a new
    landmark arrives with its first sighting, placed by it); every 60th call is april_graph_cholesky.  -> chi2 per call, fall-back flags, per call (polar arrived, re-planned)"""
    fa, fb, z, W = d["plain"]
    n = d["n_poses"]
    g = lib.new_graph(); p = lib.new_param(nthreshold=100)
    lib.clear_error()
    node = {}
    chi, was_batch, info = [], [], []

    def step(polar_arrived):
        if len(chi) % 60 == 0:                  # (the first call, and a caller-made fall-back at every 60th: a batch step on the grown graph)
            g.cholesky(p); was_batch.append(True); info.append((polar_arrived, 1))
        else:
            p.c.batch_time = 1e300
            bt = p.c.batch_time
            g.cholesky_inc(p)
            was_batch.append(p.c.batch_time != bt)
            info.append((polar_arrived, p.stats()["inc_replanned"]))
        assert p.stats()["not_spd"] == 0 and lib.last_error()[0] == 0, (len(chi), lib.last_error())
        chi.append(g.chi2())

    for i in range(n):
        for what, k in d["events"][i]:
            if len(chi) >= steps:
                break
            if what == "node" and k < n:
                node[k] = g.add_node_xyt(d["start"][0] if k == 0 else _compose(g.states_of(node[k - 1]), z[k]))      # (plain factor k: odometry k-1 -> k)
            elif what == "plain":
                if fb[k] < 0:
                    g.add_factor_xytpos(node[int(fa[k])], z[k], W[k].reshape(3, 3))
                else:
                    g.add_factor_xyt(node[int(fa[k])], node[int(fb[k])], z[k], W[k].reshape(3, 3))
                step(False)
            elif what == "polar":
                kind, a, b, zz, WW = d["polars"][k]
                if b not in node:                                    # (first sighting: range and bearing)
                    pa = g.states_of(node[a])
                    node[b] = g.add_node_xyt([pa[0] + zz[0] * np.cos(pa[2] + zz[1]), pa[1] + zz[0] * np.sin(pa[2] + zz[1]), 0.0])
                    # nothing observes a landmark's heading, and an incremental step puts no Tikhonov term on the nodes it adds
                    # (aprilsam.c:508-542): the heading prior of include/aprilsam_amd.h
                    g.add_factor_xytpos(node[b], [0.0, 0.0, 0.0], np.diag([0.0, 0.0, 1.0]))
                g.add_factor_polar(kind, node[a], node[b], zz, WW)
                step(True)
    out = dict(chi=np.array(chi), was_batch=np.array(was_batch), info=info, states=g.states())
    p.destroy(); g.destroy()
    return out


def test_incremental_run_against_host_evaluated(lib):
    d = pm.snake(10, 14, seed=3)
    assert d["plain"][1][0] < 0 and np.array_equal(d["plain"][1][1:], np.arange(1, d["n_poses"]))      # plain factor k: the odometry into pose k
    steps = 306                                                     # 6 batch steps (the first call and every 60th) and 300 incremental ones
    a = _grow(lib, d, steps)
    with lib.options(polar_on_host=1):
        b = _grow(lib, d, steps)
    assert len(a["chi"]) == steps == len(b["chi"])
    assert np.array_equal(a["was_batch"], b["was_batch"])           # identical fall-back schedule
    err = np.abs(a["chi"] - b["chi"]) / np.maximum(1.0, np.abs(b["chi"]))
    print(f"incremental run: chi2 per step, native against host-evaluated: worst {err.max():.3e}; fall-backs {int(a['was_batch'].sum())}")
    assert err.max() <= 1e-6, err.max()
    fast = [k for k in range(1, steps) if a["info"][k][0] and not a["was_batch"][k] and a["info"][k][1] == 0]
    batch = [k for k in range(1, steps) if a["info"][k][0] and a["was_batch"][k]]
    replanned = [k for k in range(1, steps) if a["info"][k][0] and not a["was_batch"][k] and a["info"][k][1] == 1]
    print(f"polar factors arriving on fast-path steps: {len(fast)}, on batch fall-backs: {len(batch)}, on re-planned incremental steps: {len(replanned)}")
    assert len(fast) >= 1 and len(batch) + len(replanned) >= 1
    assert int((~a["was_batch"]).sum()) == 300 and len(batch) >= 1 and len(replanned) >= 1
    assert all(i[1] == 1 for i in b["info"][1:])                      # (host-evaluated factors never take the fast path)


# ---- 8. consumers of the retained factor ----------------------------------------------------------------------------------------
def test_consumers_against_the_dense_inverse(lib, medium):
    d = medium
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    g.cholesky(p)
    lp = g.l_points()
    assert np.array_equal(lp, d["start"])
    A, _ = pm.system(lp, d["plain"], d["polars"], pm.TIKHANOV)
    S = np.linalg.inv(A.toarray())
    N = len(lp)
    blk = lambda i, j: S[3 * i:3 * i + 3, 3 * j:3 * j + 3]
    cov = g.marginals(p)
    _close(cov.reshape(N, 3, 3), np.array([blk(i, i) for i in range(N)]), "marginals")
    rng = np.random.default_rng(1)
    a = rng.integers(0, N, 12).astype(np.int32); b = rng.integers(0, N, 12).astype(np.int32)
    b[0], b[1] = a[0], N - 1                                         # (a == b, and a landmark)
    J = np.asarray(g.marginals_joint_any(p, a, b)).reshape(len(a), 6, 6)
    want = np.array([np.block([[blk(i, i), blk(i, j)], [blk(j, i), blk(j, j)]]) for i, j in zip(a, b)])
    _close(J, want, "marginals_joint_any")
    # gate_xyt on xyt candidates between poses
    n = d["n_poses"]
    ga = rng.integers(0, n, 6).astype(np.int32); gb = (ga + rng.integers(1, n - 1, 6)).astype(np.int32) % n
    zc = rng.normal(0, 1, (6, 3)); Wc = np.tile(np.diag([100.0, 100.0, 400.0]).reshape(9), (6, 1))
    st = g.states()
    d2, Sg = g.gate_xyt(p, ga, gb, zc, Wc)
    from tests.support.normal_eq import linearise
    Ja, Jb, r = linearise(st, ga, gb, zc)
    for k in range(6):
        Jk = np.hstack([Ja[k], Jb[k]])
        P = np.block([[blk(ga[k], ga[k]), blk(ga[k], gb[k])], [blk(gb[k], ga[k]), blk(gb[k], gb[k])]])
        Sk = Jk @ P @ Jk.T + np.linalg.inv(Wc[k].reshape(3, 3))
        _close(np.asarray(Sg).reshape(6, 3, 3)[k], Sk, f"gate_xyt S of candidate {k}")
        _close(np.asarray(d2)[k], r[k] @ np.linalg.solve(Sk, r[k]), f"gate_xyt d2 of candidate {k}")
    B = rng.normal(0, 1, (3, 3 * N))
    X = g.solve(p, B, mode="full")
    _close(np.asarray(X).reshape(3, 3 * N), (S @ B.T).T, "solve FULL")
    p.destroy(); g.destroy()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_param_alone(lib, small, tmp_path):
    d = small
    fresh = pm.build(lib, d["start"], d["plain"], d["polars"]); pf = lib.new_param()
    fresh.cholesky(pf)
    want = fresh.states()
    g = pm.build(lib, d["start"], d["plain"], d["polars"]); p = lib.new_param()
    st0 = g.states()
    ipol = len(d["plain"][0])                                        # the first polar factor
    dll = lib.dll
    # a loss on a polar factor
    lib.clear_error()
    assert g.set_robust(ipol, abi.ROBUST_CAUCHY, 1.0) == -12 and lib.last_error()[0] == -12
    # a polar factor as a max component
    comp = g.make_factor_polar(pm.RANGE, 0, 1, [1.0], [2.0])
    arr = (C.POINTER(abi.Factor) * 1)(comp)
    assert not dll.aprilsam_amd_factor_max_create(arr, host._np_d(np.zeros(1)), 1) and lib.last_error()[0] == -12
    abi.destroy_factor(comp)
    # a polar factor as a GNC candidate: weights and trace untouched
    o = abi.GncOpts(); dll.aprilsam_amd_gnc_opts_init(C.byref(o))
    rep = abi.GncReport(); rep.status = -77
    w = np.full(2, -7.0); tr = np.full(4 * o.max_stages, -7.0)
    cand = np.array([1, ipol], np.int32)
    lib.clear_error()
    assert dll.aprilsam_amd_optimize_gnc(g.ptr, p.ptr, C.byref(o), 2, host._np_i(cand), C.byref(rep), host._np_d(w), host._np_d(tr)) == -12
    assert lib.last_error()[0] == -12 and np.all(w == -7.0) and np.all(tr == -7.0) and rep.status == -77
    # chordal initialisation on a graph that holds one
    co = abi.ChordalOpts(); dll.aprilsam_amd_chordal_opts_init(C.byref(co))
    crep = abi.ChordalReport(); crep.status = -77
    rot = np.full(2 * g.n_nodes, -7.0)
    lib.clear_error()
    assert dll.aprilsam_amd_initialize_chordal(g.ptr, p.ptr, C.byref(co), C.byref(crep), host._np_d(rot)) == -12
    assert lib.last_error()[0] == -12 and np.all(rot == -7.0) and crep.status == -77
    # sharded runs
    dll.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    ps = lib.new_param()
    lib.clear_error()
    assert dll.aprilsam_amd_shard_begin(C.cast(g.ptr, C.c_void_p), C.cast(ps.ptr, C.c_void_p), 0, 1) == -12 and lib.last_error()[0] == -12
    ps.destroy()
    # .graph files
    path = tmp_path / "p.graph"
    assert g.save(str(path)) is False and not path.exists()
    # a polar factor's W edited into an indefinite one: -12 at the next call, states untouched
    Wd = C.cast(C.cast(g.factor(ipol).u.W, C.c_void_p).value + 8, C.POINTER(C.c_double))
    keep = Wd[0]
    Wd[0] = -keep
    lib.clear_error()
    g.cholesky(p)
    assert lib.last_error()[0] == -12 and np.array_equal(g.states(), st0)
    Wd[0] = keep
    # nothing was written, and the param is as usable as one that never saw a refused call
    assert np.array_equal(g.states(), st0) and np.array_equal(g.l_points(), st0)
    g.cholesky(p)
    assert g.states().tobytes() == want.tobytes()
    for gg, pp in ((g, p), (fresh, pf)):
        pp.destroy(); gg.destroy()
