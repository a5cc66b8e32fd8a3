"""Dense Gaussian factors on the GPU: the slots k_gaussian_slot writes, read back through the assembled system of
aprilsam_amd_debug_stage and compared with the numpy model (k = 1, 2, 3, 11; both orientations of the off-diagonal slot; the heading
wrap); the host-evaluated clique (option gaussian_on_host) as the A/B oracle of a step; the normal equations of a step with a
rank-deficient factor on a handful of kernel paths; chi^2 through april_graph_chi2, the resident loop and LM; the capture keys; LM, GNC and
the resident loop against repeated batch calls; fixed nodes; and every refusal.

Tolerances: ten times what the float64 model deviates from the longdouble model on the same input (DESIGN.md section 24 records the
figures the tests print); the normal equations: ten times what the same graph WITHOUT the Gaussian factor reaches on the same path."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import abi
from tests.support import gaussian_graphs as gg
from tests.support import marginal_prior_model as mm
from tests.support.kernel_paths import KERNEL_PATHS

pytestmark = pytest.mark.gpu
LAM = 1e-4          # april_graph_cholesky_param_init's tikhanov


def _relative(seed, nodes, pts, name="relative"):
    """a Gaussian factor of the given rank class on `nodes` with xbar near pts"""
    rng = np.random.default_rng(seed)
    xbar, eta, Lam = gg.random_gaussian(rng, name, len(nodes))
    xbar = pts[list(nodes)] + rng.normal(0, 0.05, (len(nodes), 3))
    return (list(nodes), xbar, eta, Lam)


def _dev(a64, ald):
    return float(np.max(np.abs(np.asarray(a64, np.longdouble) - ald), initial=0.0))


SLOT_CASES = {
    "k1": (6, (2,), "regular"), "k2": (6, (1, 4), "relative"), "k2_swapped": (6, (4, 1), "relative"), "k3": (6, (4, 1, 3), "relative"),
    "k3_regular": (6, (0, 5, 2), "regular"), "k11": (12, (7, 0, 11, 3, 9, 1, 5, 10, 2, 8, 4), "relative"), "wrap": (12, (3, 9), "regular"),
}


def _slot_scene(case):
    n, nodes, name = SLOT_CASES[case]
    # (wrap: a snake that turns right by 0.344 per pose heads -3.096 at pose 9; the factor's xbar there is +3.1: delta is 0.087, not -6.196)
    sc = gg.snake(n, 11, closures=[(0, n - 1)], **(dict(turn=-0.344, noise=0.01) if case == "wrap" else {}))
    ga = _relative(12, nodes, sc["start"], name)
    if case == "wrap":
        assert -3.13 < sc["start"][9, 2] < -3.06
        ga[1][1, 2] = 3.1
    return sc, ga


# ---- 1. slots ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(SLOT_CASES))
def test_slots_against_the_model(lib, case):
    sc, ga = _slot_scene(case)
    g = gg.build(lib, sc, [ga]); p = lib.new_param()
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    if case == "wrap":             # (the step pulls pose 9 across: the system is assembled where its heading is -3.096 and xbar's +3.1)
        g.set_all_states(sc["start"])
    st = g.states()
    if case == "wrap":
        assert st[9, 2] < -3.0 and ga[1][1, 2] == 3.1 and abs(mm.gaussian_delta(st, ga[0], ga[1])[5] - (st[9, 2] - 3.1 + 2 * np.pi)) < 1e-12
    A, B = gg.assembled(lib, g, p)
    A64, B64 = gg.model_system(sc, st, [ga], LAM)
    Al, Bl = gg.model_system(sc, st, [ga], LAM, np.longdouble)
    for what, got, m64, ml in (("A", A, A64, Al), ("B", B, B64, Bl)):
        allowed, err = 10 * _dev(m64, ml), _dev(got, ml)
        print(f"gaussian slots {case} {what}: |device - longdouble| = {err:.3e}, allowed 10 x |float64 - longdouble| = {allowed:.3e}")
        assert err <= allowed, (case, what, err, allowed)
    # a wrong orientation bit or carry bit is not a rounding matter: the factor's own blocks, against Lambda itself
    rows = mm._rows(ga[0])
    A0, _ = gg.model_system(sc, st, [], LAM, np.longdouble)
    assert _dev(A[np.ix_(rows, rows)] - ga[3], A0[np.ix_(rows, rows)]) <= 10 * _dev(A64, Al) + 1e-300
    p.destroy(); g.destroy()


@pytest.mark.parametrize("case", list(SLOT_CASES))
def test_host_evaluated_clique_gives_the_same_step(lib, case):
    sc, ga = _slot_scene(case)
    dx = {}
    for host in (0, 1):
        with lib.options(gaussian_on_host=host):
            g = gg.build(lib, sc, [ga]); p = lib.new_param()
            g.cholesky(p)
            assert p.stats()["not_spd"] == 0
            dx[host] = g.deltas().copy()
            p.destroy(); g.destroy()
    d64 = gg.model_step(sc, sc["start"], [ga], LAM)
    dl = gg.model_step(sc, sc["start"], [ga], LAM, np.longdouble)
    allowed = 10 * _dev(d64, dl)
    for host in (0, 1):
        err = _dev(dx[host], dl)
        print(f"gaussian step {case} on_host={host}: |device - longdouble| = {err:.3e}, allowed {allowed:.3e}")
        assert err <= allowed, (case, host, err, allowed)
    assert _dev(dx[0], dx[1].astype(np.longdouble)) <= allowed


# ---- 2. normal equations ---------------------------------------------------------------------------------------------------------------
PATHS = [KERNEL_PATHS[0], KERNEL_PATHS[-1], dict(use_graph=0), dict(linearize_staged_min=0), dict(persist=0)]


@pytest.mark.parametrize("opts", PATHS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_step_with_a_rank_deficient_factor_satisfies_the_normal_equations(lib, opts):
    sc = gg.snake(30, 21, closures=[(0, 29), (4, 20), (9, 17)])
    ga = _relative(22, (25, 3, 14, 8), sc["start"])
    rel = {}
    with lib.options(**opts):
        for tag, gauss in (("without", []), ("with", [ga])):
            g = gg.build(lib, sc, gauss); p = lib.new_param()
            worst = 0.0
            for _ in range(2):
                g.cholesky(p)
                assert p.stats()["not_spd"] == 0
                worst = max(worst, gg.normal_eq_rel(sc, g.l_points(), g.deltas(), gauss, LAM))
            rel[tag] = worst
            p.destroy(); g.destroy()
    print(f"gaussian normal equations {opts}: without the factor {rel['without']:.3e}, with it {rel['with']:.3e}")
    assert rel["with"] <= 10 * rel["without"], rel


# ---- 3. chi^2 ------------------------------------------------------------------------------------------------------------------------
def test_chi2_api_resident_and_lm(lib):
    sc = gg.snake(12, 31, closures=[(0, 11), (2, 8)])
    gauss = [_relative(32, (7, 2, 10), sc["start"]), _relative(33, (5,), sc["start"], "regular"), _relative(34, (9, 4), sc["start"], "zero")]
    rng = np.random.default_rng(35)
    g = gg.build(lib, sc, gauss); p = lib.new_param()
    moved = sc["start"] + rng.normal(0, 0.2, sc["start"].shape)
    g.set_all_states(moved)
    want, terms = gg.model_chi2(sc, moved, gauss)
    assert all(t >= 0 for t in terms) and terms[0] > 0 and terms[2] == 0
    got = g.chi2()
    assert abs(got - want) <= 1e-12 * want, (got, want)
    d = lib.dll
    d.aprilsam_amd_resident_chi2.restype = C.c_double
    assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    assert abs(d.aprilsam_amd_resident_chi2(g.ptr) - want) <= 1e-12 * want
    assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    # at xbar with eta = 0 the term is exactly c0 = 0, never negative
    z = gg.build(lib, dict(sc, start=sc["start"]), [(gauss[0][0], sc["start"][gauss[0][0]], np.zeros(9), gauss[0][3])])
    base = gg.model_chi2(sc, sc["start"], [])[0]
    assert z.chi2() >= base * (1 - 1e-15) and abs(z.chi2() - base) <= 1e-12 * base
    z.destroy()
    # LM's objective counts the full r'Wr of every factor and the Gaussian terms
    r = g.optimize_lm(p, max_iters=1, trace=True)
    wantF = gg.model_chi2(sc, moved, gauss, halves=False)[0]
    assert abs(r["F_initial"] - wantF) <= 1e-12 * wantF, (r["F_initial"], wantF)
    st = g.states()
    wantF1 = gg.model_chi2(sc, st, gauss, halves=False)[0]
    assert abs(r["F_final"] - wantF1) <= 1e-11 * max(wantF1, 1.0), (r["F_final"], wantF1)
    p.destroy(); g.destroy()


# ---- 4. capture keys -------------------------------------------------------------------------------------------------------------------
def test_added_and_edited_factor_between_replays(lib):
    sc = gg.snake(14, 41, closures=[(0, 13)])
    ga = _relative(42, (3, 9, 6), sc["start"])
    g = gg.build(lib, sc); p = lib.new_param()
    for _ in range(3):
        g.cholesky(p)
    n0 = p.graph_captures()
    assert n0 >= 1
    g.cholesky(p)
    assert p.graph_captures() == n0                                # a replay
    gauss = [ga]
    i = g.add_factor_gaussian(*ga)
    for k in range(3):
        lp = g.states().copy()
        g.cholesky(p)
        assert gg.normal_eq_rel(sc, lp, g.deltas(), gauss, LAM) < 1e-10
    assert p.graph_captures() > n0                                 # the new table and the new entries: captured again
    f = g.factor(i)
    n = 3 * len(ga[0])
    f.u.z[n + 1] += 0.75                                           # eta[1], in place: the table is uploaded again where it lies
    eta2 = ga[2].copy(); eta2[1] += 0.75
    edited = [(ga[0], ga[1], eta2, ga[3])]
    for k in range(2):
        lp = g.states().copy()
        g.cholesky(p)
        assert gg.normal_eq_rel(sc, lp, g.deltas(), edited, LAM) < 1e-10
        assert gg.normal_eq_rel(sc, lp, g.deltas(), gauss, LAM) > 1e-6      # (not the step of the factor before the edit)
    p.destroy(); g.destroy()


# ---- 5. optimisers, the resident loop, fixed nodes -------------------------------------------------------------------------------------
def _opt_scene():
    sc = gg.snake(16, 51, closures=[(0, 15), (3, 12), (6, 10)])
    return sc, [_relative(52, (13, 2, 8), sc["start"]), _relative(53, (5, 11), sc["start"], "regular")]


def test_resident_loop_agrees_with_batch_calls(lib):
    sc, gauss = _opt_scene()
    ga = gg.build(lib, sc, gauss); pa = lib.new_param()
    for _ in range(3):
        ga.cholesky(pa)
    gr = gg.build(lib, sc, gauss); pr = lib.new_param()
    chi2, _ = gr.batch_resident(pr, 3)
    assert np.max(np.abs(gr.states() - ga.states())) < 1e-11
    assert abs(chi2[-1] - ga.chi2()) <= 1e-10 * max(1.0, ga.chi2())
    assert abs(chi2[0] - gg.model_chi2(sc, sc["start"], gauss)[0]) <= 1e-12 * chi2[0]
    for x in (pa, pr):
        x.destroy()
    ga.destroy(); gr.destroy()


def test_lm_converges_to_the_model_s_minimum(lib):
    sc, gauss = _opt_scene()
    g = gg.build(lib, sc, gauss); p = lib.new_param()
    p.c.tikhanov = 0.0
    r = g.optimize_lm(p, max_iters=60)
    assert r["status"] in (1, 2, 3) and r["F_final"] < r["F_initial"]      # (a stop test, not the iteration limit)
    st = g.states()
    A, B = gg.model_system(sc, st, gauss, 0.0, np.longdouble)      # the gradient of the objective at the minimum
    scale = float(np.max(np.abs(A) @ np.ones(len(B))))
    assert float(np.max(np.abs(B))) < 1e-5 * scale
    assert abs(r["F_final"] - gg.model_chi2(sc, st, gauss, halves=False)[0]) <= 1e-10 * max(1.0, r["F_final"])
    p.destroy(); g.destroy()


def test_gnc_with_the_factor_as_a_non_candidate(lib):
    sc, gauss = _opt_scene()
    cand = [16, 17, 18]                                            # the three closures (factor 0: the prior, 1 .. 15: odometry)
    g = gg.build(lib, sc, gauss); p = lib.new_param()
    r = g.optimize_gnc(p, cand, c=1000.0, max_stages=8, max_iters=30)
    assert r["stages"] >= 1 and np.all(np.isfinite(g.states())) and np.all(r["weights"] > 0.999)
    # a scale far above every residual: the surrogate is the plain cost, the outcome the fixed point of repeated batch calls
    h = gg.build(lib, sc, gauss); q = lib.new_param()
    for _ in range(12):
        h.cholesky(q)
    assert np.max(np.abs(h.states() - g.states())) < 1e-4
    lib.clear_error()
    with pytest.raises(Exception):
        g.optimize_gnc(p, [19], c=3.0)                             # the Gaussian factor as a candidate
    assert lib.last_error()[0] == -12
    for x in (p, q):
        x.destroy()
    g.destroy(); h.destroy()


def test_fixed_node_masks_the_factor_s_entries(lib):
    sc, gauss = _opt_scene()
    g = gg.build(lib, sc, gauss); p = lib.new_param()
    assert g.set_fixed(2) == 0 and g.set_fixed(11) == 0
    before = g.states().copy()
    g.cholesky(p)
    dx = g.deltas()
    # (x and y bit for bit; the heading goes through the update's mod2pi, as tests/test_gpu_fixed.py notes)
    assert np.array_equal(g.states()[[2, 11], :2], before[[2, 11], :2]) and np.max(np.abs(g.states()[[2, 11], 2] - before[[2, 11], 2])) < 1e-15
    assert not dx[[2, 11]].any()
    A, B = gg.model_system(sc, before, gauss, LAM, np.longdouble)
    free = mm._rows([i for i in range(16) if i not in (2, 11)])
    want = mm.solve_spd(A[np.ix_(free, free)], B[free], np.longdouble)
    w64 = mm.solve_spd(A[np.ix_(free, free)].astype(float), B[free].astype(float))
    assert _dev(dx.reshape(-1)[free], want) <= 10 * _dev(w64, want)
    p.destroy(); g.destroy()


def test_marginals_and_solve_see_the_factor(lib):
    sc, gauss = _opt_scene()
    g = gg.build(lib, sc, gauss); p = lib.new_param()
    lp = g.states().copy()
    g.cholesky(p)
    A, _ = gg.model_system(sc, lp, gauss, LAM)
    S = np.linalg.inv(A)
    cov = g.marginals(p, [2, 8, 13])
    for k, i in enumerate((2, 8, 13)):
        blk = S[3 * i:3 * i + 3, 3 * i:3 * i + 3]
        assert np.max(np.abs(cov[k] - blk)) < 1e-9 * np.max(np.abs(blk))
    rhs = np.random.default_rng(54).normal(size=48)
    assert np.max(np.abs(g.solve(p, rhs) - S @ rhs)) < 1e-9 * np.max(np.abs(S @ rhs))
    p.destroy(); g.destroy()


# ---- 6. refusals and the audit ---------------------------------------------------------------------------------------------------------
def test_incremental_entry_points_refuse(lib):
    sc, gauss = _opt_scene()
    g = gg.build(lib, sc, gauss); p = lib.new_param()
    g.cholesky(p)
    g.add_factor_xyt(1, 9, [0.5, 0.5, 0.1], np.eye(3))
    before = (g.states().copy(), g.l_points().copy(), g.deltas().copy())
    for call, who in ((g.cholesky_inc, "april_graph_cholesky_inc"), (g.cholesky_inc_solver, "april_graph_cholesky_inc_solver")):
        lib.clear_error()
        call(p)
        code, msg = lib.last_error()
        assert code == -12 and who in msg and "Gaussian" in msg, (code, msg)
        assert np.array_equal(g.states(), before[0]) and np.array_equal(g.l_points(), before[1]) and np.array_equal(g.deltas(), before[2])
    g.cholesky(p)                                                  # the param kept its plan: a batch call goes on
    assert p.stats()["not_spd"] == 0
    p.destroy(); g.destroy()


def test_chordal_initialisation_refuses(lib):
    sc, gauss = _opt_scene()
    g = gg.build(lib, sc, gauss); p = lib.new_param()
    before = g.states().copy()
    lib.clear_error()
    with pytest.raises(Exception):
        g.initialize_chordal(p)
    code, msg = lib.last_error()
    assert code == -12 and "Gaussian" in msg and np.array_equal(g.states(), before)
    p.destroy(); g.destroy()


def test_edit_that_breaks_lambda_fails_the_call(lib):
    sc, gauss = _opt_scene()
    g = gg.build(lib, sc, gauss); p = lib.new_param()
    g.cholesky(p)
    before = g.states().copy()
    f = g.factor(g.n_factors - 1)
    Wd = C.cast(C.cast(f.u.W, C.c_void_p).value + 8, C.POINTER(C.c_double))
    keep = Wd[0]
    Wd[0] = -1.0
    lib.clear_error()
    g.cholesky(p)
    assert lib.last_error()[0] == -12 and np.array_equal(g.states(), before)
    Wd[0] = keep
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0 and not np.array_equal(g.states(), before)
    p.destroy(); g.destroy()


def test_audit_counts_it_as_unavailable_and_audits_the_rest_unchanged(lib):
    sc = gg.snake(16, 51, closures=[(0, 15), (3, 12), (6, 10)])
    zero = (list((5, 11)), sc["start"][[5, 11]], np.zeros(6), np.zeros((6, 6)))      # a factor that changes nothing: the rest must not move
    g0 = gg.build(lib, sc); p0 = lib.new_param()
    g0.cholesky(p0); g0.cholesky(p0)
    a0, n0 = g0.factor_audit(p0)
    g1 = gg.build(lib, sc, [zero, _relative(55, (2, 9, 13), sc["start"], "zero")]); p1 = lib.new_param()
    g1.cholesky(p1); g1.cholesky(p1)
    a1, n1 = g1.factor_audit(p1)
    F = len(sc["fa"])
    assert n0 == 0 and n1 == 2 and np.isnan(a1[F:]).all() and a1.shape == (F + 2, 4)
    assert a1[:F].tobytes() == a0.tobytes() or np.max(np.abs(a1[:F] - a0)) <= 1e-9 * np.max(np.abs(a0))
    for x in (p0, p1):
        x.destroy()
    g0.destroy(); g1.destroy()
