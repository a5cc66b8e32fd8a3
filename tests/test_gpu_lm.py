"""aprilsam_amd_optimize_lm on the GPU: parity with the numpy model (tests/support/lm_model.py), monotone F,
the divergence the plain step shows from a bad start, the optimum, determinism, the contract it leaves behind, and every refusal."""
import numpy as np
import pytest

from aprilsam_amd import datasets
from aprilsam_amd.host import LMError, MarginalsError
from tests.support import lm_model as M
from tests.support import maxmix_model
from tests.support.normal_eq import normal_equation_residual

pytestmark = pytest.mark.gpu

RES_RTOL = 1e-10        # tests/test_gpu_normal_eq.py


def _graph(lib, states, fa, fb, z, W):
    g = lib.new_graph(); g.build_from_arrays(states, fa, fb, z, W)
    return g


def _ang(a, b):
    d = a - b
    d[:, 2] = M.mod2pi(d[:, 2])
    return np.abs(d).max()


def _m3500(sigma=None):
    st, fa, fb, z, W = datasets.m3500_batch()
    return (M.perturbed(st, sigma) if sigma else st), (fa, fb, z, W)


def _random(seed):
    st, fa, fb, z, W = datasets.random_pose_graph(300, 200, seed)
    return M.perturbed(st, 0.5, seed), (fa, fb, z, W)


CASES = [("random%d" % s, (lambda s=s: _random(s)), 50) for s in range(4)] + [("m3500_s0.3", lambda: _m3500(0.3), 50),
                                                                               ("m3500_s1.0", lambda: _m3500(1.0), 20)]


def _accepted_monotone(r):
    acc = r["trace"][r["trace"][:, 3] == 1, 0]
    return bool(np.all(np.diff(np.concatenate([[r["F_initial"]], acc])) <= 0))


def _parity_with_the_model(lib, x0, plain, iters, name="", **lm_opts):
    """aprilsam_amd_optimize_lm against tests/support/lm_model.py under the library options in force: decisions exact, lambda at 1e-6,
    F and the states at 1e-9.  Returns the trace and the final states"""
    ref = M.optimize(x0, plain, max_iters=iters)
    g = _graph(lib, x0, *plain); p = lib.new_param()
    r = g.optimize_lm(p, trace=True, max_iters=iters, **lm_opts)
    assert abs(r["F_initial"] - ref["F_initial"]) <= 1e-12 * abs(ref["F_initial"])
    n = M.comparable_rows(ref["trace"], ref["F_initial"])
    assert n >= 1, name
    t, rt = r["trace"], ref["trace"]
    assert len(t) >= n
    assert np.array_equal(t[:n, 3], rt[:n, 3]), (name, t[:n, 3], rt[:n, 3])
    # lambda follows rho = (F - F_t) / pred, whose rounding grows as F - F_t shrinks (1e-13 of F over a decrease of 1e-6 F is 1e-7 of
    # rho): lambda is compared at 1e-6 while the decrease stays above 1e-7 F, the decisions exactly
    nl = M.comparable_rows(rt, ref["F_initial"], f_band=1e-7)
    assert np.all(np.abs(t[:nl, 2] - rt[:nl, 2]) <= 1e-6 * np.abs(rt[:nl, 2])), (name, np.max(np.abs(t[:nl, 2] / rt[:nl, 2] - 1)))
    assert np.all(np.abs(t[:n, 0] - rt[:n, 0]) <= 1e-9 * np.abs(rt[:n, 0])), name
    if len(t) == len(rt) and np.array_equal(t[:, 3], rt[:, 3]):
        assert r["status"] == ref["status"] and r["accepted"] == ref["accepted"]
        assert _ang(g.states(), ref["x"]) < 1e-9, (name, _ang(g.states(), ref["x"]))
    # the states after the comparable prefix (trial buffer and commit): a run cut at n iterations against the model's x after n
    gn = _graph(lib, x0, *plain); pn = lib.new_param()
    rn = gn.optimize_lm(pn, trace=True, max_iters=n, **lm_opts)
    assert rn["iterations"] == n and rn["trace"].tobytes() == t[:n].tobytes()
    assert _ang(gn.states(), ref["xs"][n - 1]) < 1e-9, (name, n, _ang(gn.states(), ref["xs"][n - 1]))
    pn.destroy(); gn.destroy()
    assert _accepted_monotone(r), name
    assert r["iterations"] <= iters and r["status"] in (1, 2, 3, 4)
    out = (r["trace"].copy(), g.states())
    p.destroy(); g.destroy()
    return out


@pytest.mark.parametrize("name,make,iters", CASES, ids=[c[0] for c in CASES])
def test_parity_with_the_model(lib, name, make, iters):
    x0, plain = make()
    _parity_with_the_model(lib, x0, plain, iters, name)


# The iteration under the batch step's kernel paths: without its captured graph (use_graph=0, alone and with stop tests every 7th
# iteration), fronts on the multi-workgroup and panel paths, both back-substitution forms, per-level launches, unplaced fronts, and the
# front pool poisoned / guard-banded before every factorisation -- a rejected step re-factorises over the previous step's numbers.
LM_PATHS = [dict(use_graph=0), dict(small_lds_kb=0), dict(small_lds_kb=48), dict(wave_backsolve=0), dict(blk_backsolve=0, small_lds_kb=0),
            dict(persist=0), dict(xcd_place=0), dict(pool_poison=1), dict(pool_guard=64), dict(use_graph=0, check_every=7)]
# the same kernels in the same order as the default run: the trace and the states bitwise
LM_BITWISE = [dict(use_graph=0), dict(xcd_place=0), dict(pool_poison=1), dict(pool_guard=64)]


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items())


def _split(opts):
    """(library options, optimize_lm options)"""
    return {k: v for k, v in opts.items() if k != "check_every"}, {k: v for k, v in opts.items() if k == "check_every"}


@pytest.mark.parametrize("opts", LM_PATHS, ids=_ids)
@pytest.mark.parametrize("name,make,iters", [CASES[0], CASES[4]], ids=[CASES[0][0], CASES[4][0]])
def test_parity_with_the_model_on_every_path(lib, name, make, iters, opts):
    x0, plain = make()
    lo, lm = _split(opts)
    with lib.options(**lo):
        t, x = _parity_with_the_model(lib, x0, plain, iters, name, **lm)
    if opts in LM_BITWISE:
        g = _graph(lib, x0, *plain); p = lib.new_param()
        r = g.optimize_lm(p, trace=True, max_iters=iters)
        assert r["trace"].tobytes() == t.tobytes() and g.states().tobytes() == x.tobytes(), (name, opts)
        p.destroy(); g.destroy()


def _monotone_with_max_mixture_factors(lib):
    states, base, loops, outliers = maxmix_model.m3500_outliers()
    g = maxmix_model.build(lib, states, base, loops + outliers, as_max=True)
    p = lib.new_param()
    r = g.optimize_lm(p, trace=True, max_iters=60)
    assert r["status"] in (1, 2, 4) and r["accepted"] >= 1
    assert _accepted_monotone(r)
    x = g.states()
    mixes = maxmix_model.mixes_of(loops + outliers)
    assert abs(r["F_final"] - M.cost(x, tuple(np.asarray(v) for v in base), mixes)) <= 1e-9 * abs(r["F_final"])
    g.cholesky(p)
    sel = g.max_selected(p)[-len(mixes):]
    want = [maxmix_model.select(x[a], x[b], zs, Ws, lw) for a, b, zs, Ws, lw in mixes]
    assert list(sel) == want
    p.destroy(); g.destroy()
    return r["trace"].copy(), x


def test_monotone_with_max_mixture_factors(lib):
    _monotone_with_max_mixture_factors(lib)


@pytest.mark.parametrize("opts", [dict(use_graph=0), dict(small_lds_kb=0)], ids=_ids)
def test_monotone_with_max_mixture_factors_on_other_paths(lib, opts):
    with lib.options(**opts):
        t, x = _monotone_with_max_mixture_factors(lib)
    if opts in LM_BITWISE:                                      # (use_graph=0: the kernels and their order are the default run's)
        t0, x0 = _monotone_with_max_mixture_factors(lib)
        assert t.tobytes() == t0.tobytes() and x.tobytes() == x0.tobytes()


def test_plain_step_diverges_where_lm_does_not(lib):
    x0, plain = _m3500(1.0)
    g = _graph(lib, x0, *plain); p = lib.new_param(); p.c.tikhanov = 0.0
    for _ in range(20):
        g.cholesky(p)
    chi2_gn = g.chi2()
    runs = []
    for tk in (0.0, 1e-3):
        g2 = _graph(lib, x0, *plain); p2 = lib.new_param(); p2.c.tikhanov = tk
        runs.append((g2.optimize_lm(p2, trace=True, max_iters=60), g2.states(), p2.c.tikhanov))
        p2.destroy(); g2.destroy()
    (r0, s0, tk0), (r1, s1, tk1) = runs
    assert (tk0, tk1) == (0.0, 1e-3)                           # untouched
    assert chi2_gn > 100 * r0["chi2_final"], (chi2_gn, r0["chi2_final"])
    assert s0.tobytes() == s1.tobytes() and r0["trace"].tobytes() == r1["trace"].tobytes()
    p.destroy(); g.destroy()


def test_optimum_matches_undamped_gauss_newton(lib):
    x0, plain = _m3500()
    _, x_gn = M.gn_steps(x0, plain, 10, lam=0.0)
    g = _graph(lib, x0, *plain); p = lib.new_param()
    F_gn = M.cost(x_gn, plain)
    r = g.optimize_lm(p)
    assert r["status"] == 1 and r["iterations"] <= 12 and abs(r["F_final"] - F_gn) <= 1e-9 * F_gn
    # the default ftol stops where F has converged, the states to ~1e-6 (the model: 8.2e-7); a tighter ftol takes them further
    assert _ang(g.states(), x_gn) < 2e-6
    g2 = _graph(lib, x0, *plain); p2 = lib.new_param()
    r2 = g2.optimize_lm(p2, ftol=1e-15)
    assert r2["status"] in (1, 2) and _ang(g2.states(), x_gn) < 5e-8, _ang(g2.states(), x_gn)
    for o in (p, g, p2, g2):
        o.destroy()


def test_lattice_100k_converges(lib):
    st, fa, fb, z, W = lib.lattice_arrays(317)
    x0 = M.perturbed(st, 0.1)
    g = _graph(lib, x0, fa, fb, z, W); p = lib.new_param()
    r = g.optimize_lm(p, max_iters=100, ftol=1e-15)
    assert r["status"] in (1, 2), r
    g.cholesky(p)
    lp, dx = g.l_points(), g.deltas()
    out = normal_equation_residual(lp, fa, fb, z, W, dx, p.c.tikhanov)
    assert out["rel_max"] < RES_RTOL, out
    print("lattice 100k: LM", r["status"], r["iterations"], "max |dx| of the next plain step", np.abs(dx).max())
    assert np.abs(dx).max() < 1e-8, np.abs(dx).max()
    p.destroy(); g.destroy()


def test_determinism_and_check_every(lib):
    x0, plain = _m3500(1.0)
    out = []
    for ce in (1, 1, 7):
        g = _graph(lib, x0, *plain); p = lib.new_param()
        r = g.optimize_lm(p, trace=True, max_iters=30, check_every=ce)
        out.append((r, g.states().tobytes(), g.deltas().tobytes()))
        p.destroy(); g.destroy()
    for r, s, d in out[1:]:
        assert s == out[0][1] and d == out[0][2]
        assert r["trace"].tobytes() == out[0][0]["trace"].tobytes()
        assert {k: v for k, v in r.items() if k != "trace"} == {k: v for k, v in out[0][0].items() if k != "trace"}
    g = _graph(lib, x0, *plain); p = lib.new_param()
    r = g.optimize_lm(p, trace=True, max_iters=3, check_every=2)
    assert r["status"] == 4 and r["iterations"] == 3 and len(r["trace"]) == 3
    assert r["trace"].tobytes() == out[0][0]["trace"][:3].tobytes()
    p.destroy(); g.destroy()


def test_contract_and_non_interference(lib):
    x0, plain = _m3500(0.3)
    g = _graph(lib, x0, *plain); p = lib.new_param()
    g.cholesky(p)
    y0 = g.states().copy()
    dx_before = g.deltas().copy()
    # a fresh graph (and a param that never runs LM) on the same start, one step
    gr = _graph(lib, x0, *plain); pr = lib.new_param(); gr.cholesky(pr)
    assert gr.states().tobytes() == y0.tobytes()
    g.set_all_states(x0, relinearize=True)
    r = g.optimize_lm(p, trace=True)
    xs = g.states()
    assert xs.tobytes() == g.l_points().tobytes()
    acc_rows = np.nonzero(r["trace"][:, 3] == 1)[0]
    assert len(acc_rows) >= 1 and not np.isnan(g.deltas()).any() and g.deltas().tobytes() != dx_before.tobytes()
    assert p.c.tikhanov == 1e-4
    with pytest.raises(MarginalsError) as e:
        g.marginals(p)
    assert e.value.code == -1
    # incremental call after LM: as on a fresh param.  With no retained factor that is the reference's no-op (aprilsam.c:382-383:
    # april_graph_cholesky_inc returns at once without a prior factorisation), so this compares two calls that change nothing
    gf = _graph(lib, xs, *plain); pf = lib.new_param()
    g.cholesky_inc(p); gf.cholesky_inc(pf)
    assert g.states().tobytes() == gf.states().tobytes()
    # one plain step, then marginals: as a fresh param at the same states
    g.cholesky(p); gf.cholesky(pf)
    assert np.abs(g.states() - gf.states()).max() < 1e-12
    m, mf = g.marginals(p), gf.marginals(pf)
    # (the fresh param plans from other coordinates: another ordering, other rounding)
    assert np.all(np.abs(m - mf) <= 1e-6 * np.abs(mf).max(axis=(1, 2))[:, None, None]), np.max(np.abs(m - mf))
    # ... and a param with the same plan that never ran LM gives the same bits
    gr.set_all_states(xs, relinearize=True); gr.cholesky(pr)
    assert gr.states().tobytes() == g.states().tobytes() and gr.marginals(pr).tobytes() == m.tobytes()
    # the plain step on the param after LM gives the bits of a param that never ran LM
    g.set_all_states(x0, relinearize=True); gr.set_all_states(x0, relinearize=True)
    g.cholesky(p); gr.cholesky(pr)
    assert g.states().tobytes() == gr.states().tobytes() and g.deltas().tobytes() == gr.deltas().tobytes()
    g.set_all_states(x0, relinearize=True); gr.set_all_states(x0, relinearize=True)
    c1, _ = g.batch_resident(p, 3); c2, _ = gr.batch_resident(pr, 3)
    assert c1.tobytes() == c2.tobytes() and g.states().tobytes() == gr.states().tobytes()
    for o in (p, g, pr, gr, pf, gf):
        o.destroy()


def _expect(fn, code):
    with pytest.raises(LMError) as e:
        fn()
    assert e.value.code == code, e.value.code


def test_every_refusal_leaves_the_graph_and_param_usable(lib, tmp_path):
    import ctypes as C
    from tests.support import custom_scenario
    from tests.support.asym_scenarios import batch_graph
    arr = datasets.random_pose_graph(200, 100, 5)
    x0 = M.perturbed(arr[0], 0.3, 5)

    def check(g, p, code, **kw):
        s, l, d = g.states().copy(), g.l_points().copy(), g.deltas().copy()
        _expect(lambda: g.optimize_lm(p, **kw), code)
        assert lib.last_error()[0] == code
        assert s.tobytes() == g.states().tobytes() and l.tobytes() == g.l_points().tobytes() and d.tobytes() == g.deltas().tobytes()

    # bad options
    g = _graph(lib, x0, *arr[1:]); p = lib.new_param()
    for bad in (dict(max_iters=0), dict(check_every=0), dict(lambda0=-1.0), dict(eta=1.5)):
        check(g, p, -13, **bad)
    assert g.optimize_lm(p)["status"] in (1, 2)
    # host-evaluated factor
    cl = custom_scenario.build_custom_lib(str(tmp_path))
    gh = _graph(lib, x0, *arr[1:]); ph = lib.new_param()
    lib._add_factor(gh.ptr, cl.custom_heading_create(3, 0.2, 5.0))
    check(gh, ph, -4)
    gh.cholesky(ph)
    assert ph.stats()["error_code"] == 0
    # asymmetric information matrix
    ga = _graph(lib, *batch_graph()); pa = lib.new_param()
    check(ga, pa, -12)
    ga.cholesky(pa)
    assert pa.stats()["error_code"] == 0
    # sharded param
    d = lib.dll
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    d.aprilsam_amd_shard_end.argtypes = [C.c_void_p]
    gs = _graph(lib, x0, *arr[1:]); ps = lib.new_param()
    assert d.aprilsam_amd_shard_begin(C.cast(gs.ptr, C.c_void_p), C.cast(ps.ptr, C.c_void_p), 0, 1) == 0
    check(gs, ps, -12)
    d.aprilsam_amd_shard_end(C.cast(ps.ptr, C.c_void_p))
    assert gs.optimize_lm(ps)["status"] in (1, 2)
    for o in (p, g, ph, gh, pa, ga, ps, gs):
        o.destroy()
