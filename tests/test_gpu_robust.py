"""Robust losses on the GPU: identity with plain factors when every weight is 1, bitwise equivalence with a plain
graph whose W is w * W0, parity with the unmodified reference driving the independent checker factor (tests/support/robust_factor.c),
chi^2, LM against the numpy model, the 100 k lattice, edits of packed factors, a graph with max and robust factors, refusals."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from aprilsam_amd import datasets
from tests.support import lm_model
from tests.support import maxmix_model as mm
from tests.support import robust_model as rm
from tests.support.normal_eq import normal_equation_residual

pytestmark = pytest.mark.gpu
BIG = 1e150                    # c^2 = 1e300: every s of a sane graph is below it, w == 1.0 exactly


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    return rm.build_helper_lib(str(tmp_path_factory.mktemp("robust")))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), np.max(np.abs(a - b))


def _ang(a, b):
    d = a - b
    d[:, 2] = (d[:, 2] + np.pi) % (2 * np.pi) - np.pi
    return float(np.max(np.abs(d)))


def _m3500(lib, kind=None, c=BIG):
    arr = datasets.m3500_batch()
    g = lib.new_graph(); g.build_from_arrays(*arr)
    if kind is not None:
        for i in range(g.n_factors):
            assert g.set_robust(i, kind, c) == 0
    return g


def _resident(lib, g, p, steps):
    d = lib.dll
    assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, steps, 0) == 0
    assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
    chi = d.aprilsam_amd_resident_chi2(g.ptr)
    assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    return chi


# ---- 1. identity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [rm.HUBER, rm.DCS])
def test_identity_with_unit_weights(lib, kind):
    gs = [_m3500(lib), _m3500(lib, kind)]
    ps = [lib.new_param() for _ in gs]
    for it in range(3):
        chi = [g.chi2() for g in gs]
        assert chi[0] == chi[1], chi
        for g, p in zip(gs, ps):
            g.cholesky(p)
        _same(gs[0].states(), gs[1].states()); _same(gs[0].l_points(), gs[1].l_points()); _same(gs[0].deltas(), gs[1].deltas())
    w = gs[1].robust_weights(ps[1])
    assert np.all(w == 1.0) and np.all(gs[0].robust_weights(ps[0]) == -1.0)
    _same(*[g.marginals(p) for g, p in zip(gs, ps)])
    res = [g.batch_resident(p, 3) for g, p in zip(gs, ps)]
    _same(res[0][0], res[1][0]); _same(gs[0].states(), gs[1].states())
    chis = [_resident(lib, g, p, 2) for g, p in zip(gs, ps)]
    assert chis[0] == chis[1]
    _same(gs[0].states(), gs[1].states()); _same(gs[0].l_points(), gs[1].l_points())
    for g in gs:
        g.set_all_states(lm_model.perturbed(datasets.m3500_batch()[0], 0.05), relinearize=True)
    rs = [g.optimize_lm(p, trace=True, max_iters=12) for g, p in zip(gs, ps)]
    _same(rs[0]["trace"], rs[1]["trace"])
    assert {k: v for k, v in rs[0].items() if k != "trace"} == {k: v for k, v in rs[1].items() if k != "trace"}
    _same(gs[0].states(), gs[1].states())
    for g, p in zip(gs, ps):
        p.destroy(); g.destroy()


def test_identity_cauchy_then_none(lib):
    gs = [_m3500(lib), _m3500(lib, rm.CAUCHY, 0.5)]
    ps = [lib.new_param() for _ in gs]
    gs[1].cholesky(ps[1])                 # (packed with the loss, then cleared: the next call re-packs)
    gs[1].set_all_states(datasets.m3500_batch()[0], relinearize=True)
    for i in range(gs[1].n_factors):
        assert gs[1].set_robust(i, rm.NONE, 0) == 0
    for _ in range(2):
        for g, p in zip(gs, ps):
            g.cholesky(p)
        _same(gs[0].states(), gs[1].states())
    assert gs[0].chi2() == gs[1].chi2()
    for g, p in zip(gs, ps):
        p.destroy(); g.destroy()


def test_identity_incremental(lib):
    """M3500 grown through april_graph_cholesky_inc for its first 1 000 poses: plain and Huber(1e150) bitwise"""
    states, fa, fb, z, W = datasets.m3500_batch()
    order = np.argsort(np.maximum(fa, fb), kind="stable")
    gs = [lib.new_graph() for _ in range(2)]
    ps = [lib.new_param(nthreshold=100) for _ in range(2)]
    k = 0
    for n in range(1000):
        for g in gs:
            g.add_node_xyt(states[n])
        while k < len(order) and max(fa[order[k]], fb[order[k]]) <= n:
            i = order[k]; k += 1
            for w, g in enumerate(gs):
                if fb[i] < 0:
                    g.add_factor_xytpos(int(fa[i]), z[i], W[i].reshape(3, 3))
                else:
                    g.add_factor_xyt(int(fa[i]), int(fb[i]), z[i], W[i].reshape(3, 3))
                if w:
                    assert g.set_robust(g.n_factors - 1, rm.HUBER, BIG) == 0
        for g, p in zip(gs, ps):
            if n == 10:
                g.cholesky(p)
            elif n > 10:
                p.c.batch_time = 1e300
                g.cholesky_inc(p)
        if n >= 10 and (n % 50 == 0 or n == 999):
            _same(gs[0].states(), gs[1].states())
    _same(gs[0].states(), gs[1].states())
    _same(*[g.marginals(p) for g, p in zip(gs, ps)])
    for g, p in zip(gs, ps):
        p.destroy(); g.destroy()


# ---- 2. weighted-plain equivalence --------------------------------------------------------------------------------------------
def _weighted_plain_equivalence(lib, kind, c):
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(kind, c)
    gr = rm.build(lib, states, plain, kinds, cs)
    gp = lib.new_graph(); gp.build_from_arrays(states, *plain)
    pr, pp = lib.new_param(), lib.new_param()
    W0 = np.asarray(plain[3], float).reshape(-1, 9)
    for step in range(5):
        gr.cholesky(pr)
        w = gr.robust_weights(pr)
        assert np.all(w[:nb] == -1) and np.all((w[nb:] > 0) & (w[nb:] <= 1))
        We = W0.copy(); We[nb:] = w[nb:, None] * W0[nb:]
        gp.set_all_W(We)
        gp.cholesky(pp)
        _same(gr.states(), gp.states()); _same(gr.l_points(), gp.l_points()); _same(gr.deltas(), gp.deltas())
    assert np.min(w[nb:]) < 0.5
    _same(gr.marginals(pr), gp.marginals(pp))
    # resident: one step (a plain graph cannot change W in the middle of a resident run)
    for g in (gr, gp):
        g.set_all_states(states, relinearize=True)
    gp.set_all_W(W0)
    _resident(lib, gr, pr, 1)
    w = gr.robust_weights(pr)
    We = W0.copy(); We[nb:] = w[nb:, None] * W0[nb:]
    gp.set_all_W(We)
    _resident(lib, gp, pp, 1)
    _same(gr.states(), gp.states()); _same(gr.l_points(), gp.l_points())
    pr.destroy(); pp.destroy(); gr.destroy(); gp.destroy()


@pytest.mark.parametrize("kind, c", [(rm.HUBER, 1.0), (rm.CAUCHY, 1.0), (rm.DCS, 3.0)])
def test_weighted_plain_equivalence(lib, kind, c):
    _weighted_plain_equivalence(lib, kind, c)


# The weights are written into the factor slots by their own kernel before k_linearize_t reads them: the LDS-staged write-out of the
# linearisation, the per-level and no-graph forms, the multi-workgroup fronts and a new plan per call with weights other than 1.
# Tolerance-free: the robust graph and the plain graph carrying w * W0 run under the same options and agree bitwise.
BATCH_PATHS = [dict(linearize_staged_min=0), dict(use_graph=0), dict(small_lds_kb=0), dict(persist=0), dict(batch_extend=0),
               dict(linearize_staged_min=0, use_graph=0)]
INC_FORMS = [{"inc_one": 0, "inc_tail": 0}, {"inc_multi": 0}, {"inc_inline": 0}, {"inc_lazy_states": 0}, {"inc_update": 0}, {"tail_poses": 8}]


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items())


@pytest.mark.parametrize("opts", BATCH_PATHS, ids=_ids)
@pytest.mark.parametrize("kind, c", [(rm.HUBER, 1.0), (rm.CAUCHY, 1.0), (rm.DCS, 3.0)])
def test_weighted_plain_equivalence_on_other_paths(lib, kind, c, opts):
    with lib.options(**opts):
        _weighted_plain_equivalence(lib, kind, c)


# ---- 3. reference parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, c", [(rm.CAUCHY, 1.0), (rm.DCS, 3.0)])
def test_batch_parity_with_reference(lib, reflib, helper, kind, c):
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(kind, c)
    gr = rm.build(lib, states, plain, kinds, cs); pr = lib.new_param()
    gc = rm.build_checker(reflib, helper, states, plain, kinds, cs); pc = reflib.new_param()
    for step in range(10):
        gr.cholesky(pr); gc.cholesky(pc)
        assert np.max(np.abs(gr.states() - gc.states())) < 1e-8, step
    pr.destroy(); pc.destroy(); gr.destroy(); gc.destroy()


def _incremental_states(L, add, upto=1200):
    """M3500 + outliers grown pose by pose on L (Cauchy closures, each false closure inserted when its later pose arrives);
    add(g, i): adds factor i.  Returns the states at every 25th pose and at the end, and the number of robust factors added"""
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(rm.CAUCHY, 1.0)
    fa, fb, z, W = plain
    order = np.argsort(np.maximum(fa, fb), kind="stable")
    g = L.new_graph(); p = L.new_param(nthreshold=100)
    k = 0
    out = {}
    for n in range(upto):
        g.add_node_xyt(states[n])
        while k < len(order) and max(fa[order[k]], fb[order[k]]) <= n:
            add(g, order[k]); k += 1
        if n == 10:
            g.cholesky(p)
        elif n > 10:
            p.c.batch_time = 1e300
            g.cholesky_inc(p)
        if n > 10 and (n % 25 == 0 or n == upto - 1):
            out[n] = g.states()
    p.destroy(); g.destroy()
    return out, int(np.sum(kinds[order[:k]] != 0))


def _incremental_ours(lib):
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(rm.CAUCHY, 1.0)
    fa, fb, z, W = plain

    def add(g, i):
        if fb[i] < 0:
            g.add_factor_xytpos(int(fa[i]), z[i], W[i].reshape(3, 3))
        else:
            g.add_factor_xyt(int(fa[i]), int(fb[i]), z[i], W[i].reshape(3, 3))
        if kinds[i]:
            assert g.set_robust(g.n_factors - 1, int(kinds[i]), float(cs[i])) == 0
    return _incremental_states(lib, add)


@pytest.fixture(scope="module")
def incremental_reference(reflib, helper):
    """the unmodified reference driving the checker factor through the same growth (it has no options: one run serves every form)"""
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(rm.CAUCHY, 1.0)
    fa, fb, z, W = plain
    return _incremental_states(reflib, lambda g, i: rm.add_factor(reflib, helper, g, fa[i], fb[i], z[i], W[i], kinds[i], cs[i]))


def _incremental_parity(ours, ref):
    (so, no), (sr, nr) = ours, ref
    assert list(so) == list(sr) and len(so) > 40
    for n in so:
        assert _ang(so[n], sr[n]) < 1e-8, (n, _ang(so[n], sr[n]))
    assert no == nr and no > 100


def test_incremental_parity_with_reference(lib, incremental_reference):
    """M3500 + outliers grown pose by pose (Cauchy closures, each false closure inserted when its later pose arrives): both sides follow
    the same fall-back schedule and agree on the states"""
    _incremental_parity(_incremental_ours(lib), incremental_reference)


@pytest.mark.parametrize("opts", INC_FORMS, ids=_ids)
def test_incremental_parity_with_reference_under_every_launch_form(lib, incremental_reference, opts):
    """select_new_robust reads the l_point mirror or the state mirror, whichever the launch form keeps current"""
    with lib.options(**opts):
        ours = _incremental_ours(lib)
    _incremental_parity(ours, incremental_reference)


# ---- 4. chi^2 -----------------------------------------------------------------------------------------------------------------
def test_chi2_against_model(lib):
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(rm.DCS, 2.0)
    kinds = kinds.copy(); cs = cs.copy()
    kinds[0], cs[0] = rm.HUBER, 1e-3          # the prior, robust too (xytpos: rho without the 0.5)
    x = lm_model.perturbed(states, 0.02)
    g = rm.build(lib, x, plain, kinds, cs); p = lib.new_param()
    ref = rm.chi2(x, plain, kinds, cs)
    assert abs(g.chi2() - ref) <= 1e-12 * ref
    chi = _resident(lib, g, p, 2)
    # resident chi^2 at the states after the steps
    ref2 = rm.chi2(g.states(), plain, kinds, cs)
    assert abs(chi - ref2) <= 1e-12 * ref2, (chi, ref2)
    p.destroy(); g.destroy()


# ---- 5. LM --------------------------------------------------------------------------------------------------------------------
def _lm_parity_with_model(lib):
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(rm.CAUCHY, 1.0)
    x0 = lm_model.perturbed(states, 0.01)
    iters = 25
    ref = rm.optimize(x0, plain, kinds, cs, max_iters=iters)
    g = rm.build(lib, x0, plain, kinds, cs); p = lib.new_param()
    r = g.optimize_lm(p, trace=True, max_iters=iters)
    assert abs(r["F_initial"] - ref["F_initial"]) <= 1e-12 * abs(ref["F_initial"])
    n = lm_model.comparable_rows(ref["trace"], ref["F_initial"])
    assert n >= 1
    t, rt = r["trace"], ref["trace"]
    assert np.array_equal(t[:n, 3], rt[:n, 3])
    assert np.all(np.abs(t[:n, 0] - rt[:n, 0]) <= 1e-9 * np.abs(rt[:n, 0]))
    nl = lm_model.comparable_rows(rt, ref["F_initial"], f_band=1e-7)
    assert np.all(np.abs(t[:nl, 2] - rt[:nl, 2]) <= 1e-6 * np.abs(rt[:nl, 2]))
    acc = t[t[:, 3] == 1, 0]
    assert np.all(np.diff(np.concatenate([[r["F_initial"]], acc])) <= 0)
    assert abs(r["chi2_final"] - rm.chi2(g.states(), plain, kinds, cs)) <= 1e-12 * r["chi2_final"]
    # much closer to the outlier-free solution than plain LM (CPU model: tests/test_robust_host.py::test_lm_model_on_m3500_outliers)
    clean = tuple(np.asarray(v)[:nb + nl] for v in plain)
    gcl = lib.new_graph(); gcl.build_from_arrays(states, *clean); pcl = lib.new_param()
    gpl = lib.new_graph(); gpl.build_from_arrays(states, *plain); ppl = lib.new_param()
    gr = rm.build(lib, states, plain, kinds, cs); prr = lib.new_param()
    for gg, pp in ((gcl, pcl), (gpl, ppl), (gr, prr)):
        gg.optimize_lm(pp, max_iters=30)

    def err(a, b):
        d = a - b
        return float(np.mean(np.hypot(d[:, 0], d[:, 1])))
    assert err(gr.states(), gcl.states()) < 0.4 * err(gpl.states(), gcl.states())
    out = (t.copy(), g.states(), gr.states())
    for gg, pp in ((g, p), (gcl, pcl), (gpl, ppl), (gr, prr)):
        pp.destroy(); gg.destroy()
    return out


def test_lm_parity_with_model(lib):
    _lm_parity_with_model(lib)


@pytest.mark.parametrize("opts", [dict(use_graph=0), dict(small_lds_kb=0)], ids=_ids)
def test_lm_parity_with_model_on_other_paths(lib, opts):
    with lib.options(**opts):
        out = _lm_parity_with_model(lib)
    if opts == dict(use_graph=0):                                # (the kernels and their order are the default run's: the same bits)
        for v, v0 in zip(out, _lm_parity_with_model(lib)):
            _same(v, v0)


# ---- 6. scale -----------------------------------------------------------------------------------------------------------------
def test_lattice_100k_every_10th_edge_cauchy(lib):
    st, fa, fb, z, W = lib.lattice_arrays(317)
    z = z.copy()
    rng = np.random.default_rng(3)
    bad = np.arange(0, len(fa) - 1, 10)[::50]          # some of the robust edges get a wrong measurement: weights below 1
    z[bad, :2] += rng.normal(0, 1.0, (len(bad), 2))
    kinds = np.zeros(len(fa), np.int32); kinds[0:len(fa) - 1:10] = rm.CAUCHY
    cs = np.where(kinds != 0, 2.0, 0.0)
    plain = (fa, fb, z, W)
    g = rm.build(lib, st, plain, kinds, cs); p = lib.new_param()
    _resident(lib, g, p, 3)
    w = g.robust_weights(p)
    rb = kinds != 0
    assert np.all(w[~rb] == -1) and np.min(w[rb]) < 0.5
    We = np.asarray(W, float).reshape(-1, 9).copy(); We[rb] = w[rb, None] * We[rb]
    out = normal_equation_residual(g.l_points(), fa, fb, z, We, g.deltas(), 1e-4)
    assert out["rel_max"] <= 4e-12, out
    # one batch step against the plain graph with W = w * W0
    g.set_all_states(st, relinearize=True)
    g.cholesky(p)
    w = g.robust_weights(p)
    We = np.asarray(W, float).reshape(-1, 9).copy(); We[rb] = w[rb, None] * We[rb]
    gp = lib.new_graph(); gp.build_from_arrays(st, fa, fb, z, We); pp = lib.new_param()
    gp.cholesky(pp)
    _same(g.states(), gp.states())
    for gg, pq in ((g, p), (gp, pp)):
        pq.destroy(); gg.destroy()


# ---- 7. edits -----------------------------------------------------------------------------------------------------------------
def _fresh_step(lib, g, states):
    """one batch step of a copy of g's factors (kinds, W, z) from `states` on a fresh param: the reference result of an edited graph"""
    _, fa, fb, z, W = g.arrays()
    kinds = np.zeros(len(fa), np.int32); cs = np.zeros(len(fa))
    for i in range(len(fa)):
        kinds[i], cs[i] = g.get_robust(i)
    g2 = rm.build(lib, states, (fa, fb, z, W), kinds, cs); p2 = lib.new_param()
    g2.cholesky(p2)
    out = g2.states()
    p2.destroy(); g2.destroy()
    return out


@pytest.mark.parametrize("edit", ["kind", "c", "add", "remove", "W"])
def test_edit_seen_by_next_batch_call(lib, edit):
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(rm.CAUCHY, 1.0)
    g = rm.build(lib, states, plain, kinds, cs); p = lib.new_param()
    for _ in range(3):                   # warm: speculative calls and graph replay from here on
        g.cholesky(p)
        g.set_all_states(states, relinearize=True)
    i = nb + 5
    if edit == "kind":
        assert g.set_robust(i, rm.DCS, 1.0) == 0
    elif edit == "c":
        assert g.set_robust(i, rm.CAUCHY, 0.25) == 0
    elif edit == "add":
        assert g.set_robust(3, rm.HUBER, 0.01) == 0
    elif edit == "remove":
        assert g.set_robust(i, rm.NONE, 0) == 0
    else:
        Wd = g.factor(i).u.W.contents.data
        Wd[0] *= 4.0
    g.cholesky(p)
    assert _ang(g.states(), _fresh_step(lib, g, states)) < 1e-9          # (a warm param against a cold one: the same numbers to rounding)
    # resident_begin and cholesky_inc see the edit as well
    g.set_all_states(states, relinearize=True)
    assert g.set_robust(nb + 6, rm.DCS, 0.5) == 0
    _resident(lib, g, p, 1)
    assert _ang(g.states(), _fresh_step(lib, g, states)) < 1e-9
    p.destroy(); g.destroy()


# ---- 8. mixed graph -----------------------------------------------------------------------------------------------------------
def test_max_and_robust_factors_together(lib):
    states, base, loops, outl = mm.m3500_outliers()
    g = mm.build(lib, states, base, loops[:800] + outl[:25], True)           # max factors
    nmax = g.n_factors
    for a, b, zz, WW in loops[800:] + outl[25:]:
        g.add_factor_xyt(a, b, zz, np.asarray(WW).reshape(3, 3))
        assert g.set_robust(g.n_factors - 1, rm.CAUCHY, 1.0) == 0
    p = lib.new_param()
    # the model: max factors selected at x (lm_model.selected), robust ones weighted at x
    edges = loops[800:] + outl[25:]
    mixes = mm.mixes_of(loops[:800] + outl[:25])
    rob = (np.array([e[0] for e in edges]), np.array([e[1] for e in edges]), np.array([e[2] for e in edges]),
           np.array([np.asarray(e[3]).reshape(9) for e in edges]))
    x = np.array(states, float)
    for step in range(4):
        sel = lm_model.selected(x, mixes)
        We, _ = rm.w_eff(x, rob, np.full(len(edges), rm.CAUCHY), np.ones(len(edges)))
        fa = np.concatenate([base[0], sel[0], rob[0]]); fb = np.concatenate([base[1], sel[1], rob[1]])
        z = np.concatenate([np.asarray(base[2]).reshape(-1, 3), sel[2], rob[2].reshape(-1, 3)])
        W = np.concatenate([np.asarray(base[3]).reshape(-1, 9), sel[3], We])
        A, B = lm_model.system(x, fa, fb, z, W, 1e-4)
        x = lm_model.retract(x, spla.spsolve(A, B))
        g.cholesky(p)
        assert _ang(g.states(), x) < 1e-8, step
    r = g.optimize_lm(p, trace=True, max_iters=15)
    acc = r["trace"][r["trace"][:, 3] == 1, 0]
    assert np.all(np.diff(np.concatenate([[r["F_initial"]], acc])) <= 0)
    assert nmax > 0
    p.destroy(); g.destroy()


# ---- 9. refusals at solve time ------------------------------------------------------------------------------------------------
def test_refusals(lib, tmp_path):
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(rm.CAUCHY, 1.0)
    g = rm.build(lib, states, plain, kinds, cs); p = lib.new_param()
    d = lib.dll
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    st0 = g.states().copy()
    lib.clear_error()
    assert d.aprilsam_amd_shard_begin(C.cast(g.ptr, C.c_void_p), C.cast(p.ptr, C.c_void_p), 0, 1) == -12
    _same(st0, g.states())
    assert not g.save(str(tmp_path / "r.graph"))
    # a robust factor's W edited into an asymmetric one: -12 at the next call, states untouched, the param usable afterwards
    Wd = g.factor(nb + 3).u.W.contents.data
    keep = Wd[1]
    Wd[1] = keep + 1e-9
    lib.clear_error()
    g.cholesky(p)
    assert lib.last_error()[0] == -12
    _same(st0, g.states())
    Wd[1] = keep
    g.cholesky(p)
    gf = rm.build(lib, states, plain, kinds, cs); pf = lib.new_param()
    gf.cholesky(pf)
    _same(g.states(), gf.states())
    with pytest.raises(RuntimeError):
        g.robust_weights(p, [g.n_factors])
    for gg, pp in ((g, p), (gf, pf)):
        pp.destroy(); gg.destroy()


# ---- a table move with device-written weights in flight -----------------------------------------------------------------------
def test_weights_survive_a_move_of_the_table(lib):
    """tests/support/table_move.py: 140 robust factors (Cauchy) appended one or two per incremental step, 6 of them before the first
    batch step and a second batch step at the 56th.  The table is allocated for n + n / 2 + 64 rows -- 73 at the first upload -- so it
    moves when the 74th factor arrives, and every weight k_robust_weight wrote must come through: aprilsam_amd_robust_weights before and
    after every fast-path step agrees bit for bit for every older factor.  The step that takes the count past 73 is a fast-path step,
    and so are at least 90 % of all steps (a re-planned step weights everything again and proves nothing).  Checked on a scratch copy:
    with the read-back before the move deleted, this test fails (the weights of the batch steps come back as the host's stale ones)."""
    from tests.support import table_move as tm

    def add(g, a, b, z, W):
        g.add_factor_xyt(a, b, z, W)
        assert g.set_robust(g.n_factors - 1, rm.CAUCHY, 1.0) == 0
    r = tm.grow(lib, tm.scene(4), add, lambda g, p, idx: g.robust_weights(p, idx))
    print(f"robust factors {r['family']}, incremental steps {r['steps']}, fast path {r['fast']}, (step, factor) pairs compared {r['checked']}")
    assert r["family"] >= tm.FAMILY_FACTORS_MIN and r["fast"] >= 0.9 * r["steps"]
    for cap in tm.ROW_CAPS["robust"]:
        assert any(lo <= cap < hi for lo, hi in r["spans"]), (cap, r["spans"])
    assert np.all((r["values"] > 0) & (r["values"] <= 1)) and np.min(r["values"]) < 0.5 and np.max(r["values"]) > 0.9      # (Cauchy: below 1 wherever s > 0)
