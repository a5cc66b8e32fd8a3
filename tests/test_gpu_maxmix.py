"""Max-mixture factors on the GPU: parity with the unmodified reference driving the independent checker factor
(tests/support/maxmix_factor.c), K = 1 identity with plain xyt factors, replace-by-selected, incremental growth, the host path of a
foreign factor that uses tag 3, edits in place, refusals."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import abi, datasets
from tests.support import maxmix_model as mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    return mm.build_helper_lib(str(tmp_path_factory.mktemp("maxmix")))


def _wrapped_m3500(lib, wrap):
    """M3500 + prior in file order; wrap: every xyt factor as a 1-component max factor (logw 0)"""
    states, fa, fb, z, W = datasets.m3500_batch()
    g = lib.new_graph()
    g.build_from_arrays(states, fa[:0], fb[:0], z[:0], W[:0])
    for i in range(len(fa)):
        if fb[i] < 0:
            g.add_factor_xytpos(int(fa[i]), z[i], W[i].reshape(3, 3))
        elif wrap:
            g.add_factor_max(int(fa[i]), int(fb[i]), z[i:i + 1], W[i:i + 1], [0.0])
        else:
            g.add_factor_xyt(int(fa[i]), int(fb[i]), z[i], W[i].reshape(3, 3))
    return g


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), np.max(np.abs(a - b))


def test_k1_identity_batch_resident_marginals(lib):
    gs = [_wrapped_m3500(lib, w) for w in (False, True)]
    ps = [lib.new_param() for _ in gs]
    for it in range(4):
        chi = [g.chi2() for g in gs]
        assert chi[0] == chi[1], chi
        for g, p in zip(gs, ps):
            g.cholesky(p)
        _same(gs[0].states(), gs[1].states()); _same(gs[0].l_points(), gs[1].l_points()); _same(gs[0].deltas(), gs[1].deltas())
    cov = [g.marginals(p) for g, p in zip(gs, ps)]
    _same(cov[0], cov[1])
    assert np.all(gs[1].max_selected(ps[1])[1:] == 0) and gs[1].max_selected(ps[1])[0] == -1
    res = [g.batch_resident(p, 3) for g, p in zip(gs, ps)]
    _same(res[0][0], res[1][0]); _same(gs[0].states(), gs[1].states())
    d = lib.dll
    for g, p in zip(gs, ps):
        assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
        assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 2, 0) == 0
        assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
        assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    _same(gs[0].states(), gs[1].states()); _same(gs[0].l_points(), gs[1].l_points())
    _same(*[g.marginals(p) for g, p in zip(gs, ps)])
    for g, p in zip(gs, ps):
        p.destroy(); g.destroy()


def test_k1_identity_incremental(lib):
    """M3500 grown pose by pose through april_graph_cholesky_inc (fast path, low-rank updates, fall-backs): plain and wrapped bitwise"""
    states, fa, fb, z, W = datasets.m3500_batch()
    order = np.argsort(np.maximum(fa, fb), kind="stable")
    gs = [lib.new_graph() for _ in range(2)]
    ps = [lib.new_param(nthreshold=100) for _ in range(2)]
    upto = 700
    k = 0
    for n in range(upto):
        for g in gs:
            g.add_node_xyt(states[n])
        while k < len(order) and max(fa[order[k]], fb[order[k]]) <= n:
            i = order[k]; k += 1
            for w, g in enumerate(gs):
                if fb[i] < 0:
                    g.add_factor_xytpos(int(fa[i]), z[i], W[i].reshape(3, 3))
                elif w:
                    g.add_factor_max(int(fa[i]), int(fb[i]), z[i:i + 1], W[i:i + 1], [0.0])
                else:
                    g.add_factor_xyt(int(fa[i]), int(fb[i]), z[i], W[i].reshape(3, 3))
        for g, p in zip(gs, ps):
            if n == 10:
                g.cholesky(p)
            elif n > 10:
                p.c.batch_time = 1e300
                g.cholesky_inc(p)
        if n >= 10:
            _same(gs[0].states(), gs[1].states())
    _same(*[g.marginals(p) for g, p in zip(gs, ps)])
    for g, p in zip(gs, ps):
        p.destroy(); g.destroy()


def test_batch_parity_with_reference(lib, reflib, helper):
    states, base, loops, outl = mm.m3500_outliers()
    edges = loops + outl
    rec = []
    gr = mm.build(reflib, states, base, edges, True, mm.helper_adder(reflib, helper, 99, rec))
    gl = mm.build(lib, states, base, edges, True)
    pr, pl = reflib.new_param(), lib.new_param()
    nb = len(base[0])
    mixes = mm.mixes_of(edges)
    for it in range(6):
        gr.cholesky(pr); gl.cholesky(pl)
        sr = gr.states(); sl = gl.states()
        assert np.max(np.abs(sr - sl)) < 1e-9, (it, np.max(np.abs(sr - sl)))
        sel = gl.max_selected(pl)
        assert np.all(sel[:nb] == -1)
        assert np.array_equal(sel[nb:], [helper.mm_last(f) for f in rec]), it
        c = gl.chi2()
        cm = mm.chi2(sl, base, mixes)
        assert abs(c - cm) <= 1e-11 * abs(cm), (it, c, cm)
    for p in (pr, pl):
        p.destroy()
    gr.destroy(); gl.destroy()


def _replace_by_selected(lib, states, base, edges):
    gm = mm.build(lib, states, base, edges, True)
    pm = lib.new_param()
    gm.cholesky(pm)
    sel = gm.max_selected(pm)[len(base[0]):]
    assert set(sel.tolist()) == {0, 1}
    g = lib.new_graph(); fa, fb, z, W = base
    g.build_from_arrays(states, fa, fb, z, W)
    for (a, b, zz, WW), s in zip(edges, sel):
        zs, Ws, _ = mm.two_component(zz, WW)
        g.add_factor_xyt(a, b, zs[s], Ws[s].reshape(3, 3))
    p = lib.new_param()
    g.cholesky(p)
    _same(gm.states(), g.states()); _same(gm.deltas(), g.deltas())
    out = (gm.states(), sel)
    for x in (p, pm):
        x.destroy()
    g.destroy(); gm.destroy()
    return out


def test_replace_by_selected_m3500(lib):
    states, base, loops, outl = mm.m3500_outliers()
    _replace_by_selected(lib, states, base, loops + outl)


# The selected component is written into the factor slots by its own kernel before k_linearize_t reads them: the LDS-staged write-out
# of the linearisation, the per-level and no-graph forms, the multi-workgroup fronts and a new plan per call with both components
# selected.  Tolerance-free: the max-mixture graph and the plain graph of the selected components run under the same options.
BATCH_PATHS = [dict(linearize_staged_min=0), dict(use_graph=0), dict(small_lds_kb=0), dict(persist=0), dict(batch_extend=0),
               dict(linearize_staged_min=0, use_graph=0)]
INC_FORMS = [{"inc_one": 0, "inc_tail": 0}, {"inc_multi": 0}, {"inc_inline": 0}, {"inc_lazy_states": 0}, {"inc_update": 0}, {"tail_poses": 8}]


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items())


@pytest.mark.parametrize("opts", BATCH_PATHS, ids=_ids)
def test_replace_by_selected_m3500_on_other_paths(lib, opts):
    states, base, loops, outl = mm.m3500_outliers()
    with lib.options(**opts):
        _replace_by_selected(lib, states, base, loops + outl)


def test_replace_by_selected_lattice_100k(lib):
    states, fa, fb, z, W = lib.lattice_arrays(316)
    every = np.zeros(len(fa), bool); every[::10] = True; every &= fb >= 0
    base = (fa[~every], fb[~every], z[~every], W[~every])
    edges = [(int(fa[i]), int(fb[i]), z[i], W[i]) for i in np.nonzero(every)[0]]
    # (half of them false: the null hypothesis must win there)
    rng = np.random.default_rng(3)
    edges = [(a, b, zz + (rng.normal(0, 3, 3) if j % 2 else 0), WW) for j, (a, b, zz, WW) in enumerate(edges)]
    _replace_by_selected(lib, states, base, edges)


def _incremental_growth(L, add_max, selections, steps=160):
    """growth in the style of test_gpu_parity._random_growth on L: loop closures and injected outliers as max factors.
    add_max(g, a, b, zs, Ws, lw) adds one; selections(g, p) returns the components selected in every max factor so far.
    Returns the states and the selections after every step"""
    rng = np.random.default_rng(11)
    truth = [np.zeros(3)]
    g = L.new_graph(); p = L.new_param(nthreshold=12, delta_xy=0.05, delta_theta=0.05)
    g.add_node_xyt(truth[0]); g.add_factor_xytpos(0, [0, 0, 0], datasets.PRIOR_W)
    g.cholesky(p)

    def rel(a, b):
        c, s = np.cos(a[2]), np.sin(a[2]); dx, dy = b[0] - a[0], b[1] - a[1]
        return np.array([c * dx + s * dy, -s * dx + c * dy, b[2] - a[2]])

    Wl = np.diag([40.0, 40.0, 120.0])
    out = []
    for step in range(steps):
        last = truth[-1]
        new = np.array([last[0] + np.cos(last[2]) * 0.8, last[1] + np.sin(last[2]) * 0.8, last[2] + rng.uniform(-0.6, 0.6)])
        truth.append(new); n = len(truth) - 1
        init = new + rng.normal(0, [0.15, 0.15, 0.04])
        zo = rel(truth[n - 1], new) + rng.normal(0, [0.03, 0.03, 0.01])
        g.add_node_xyt(init); g.add_factor_xyt(n - 1, n, zo, Wl)
        closures = []
        if n > 4 and rng.random() < 0.5:
            o = int(rng.integers(0, n - 1))
            closures.append((o, n, rel(truth[o], truth[n]) + rng.normal(0, [0.03, 0.03, 0.01])))
        if n > 4 and step % 9 == 4:
            o = int(rng.integers(0, n - 1))
            closures.append((o, n, rng.uniform([-5, -5, -3], [5, 5, 3])))
        for a, b, zz in closures:
            zs, Ws, lw = mm.two_component(zz, Wl)
            add_max(g, a, b, zs, Ws, lw)
        p.c.batch_time = 1e300
        g.cholesky_inc(p)
        out.append((g.states(), np.array(selections(g, p))))
    p.destroy(); g.destroy()
    return out


def _incremental_ours(lib):
    def selections(g, p):
        mx = [i for i in range(g.n_factors) if g.factor(i).type == 3]
        return g.max_selected(p, mx)
    return _incremental_growth(lib, lambda g, a, b, zs, Ws, lw: g.add_factor_max(a, b, zs, Ws, lw), selections)


@pytest.fixture(scope="module")
def incremental_reference(reflib, helper):
    """the unmodified reference driving the checker factor through the same growth (it has no options: one run serves every form)"""
    rec = []
    add_ref = mm.helper_adder(reflib, helper, 99, rec)
    return _incremental_growth(reflib, add_ref, lambda g, p: [helper.mm_last(f) for f in rec])


def _incremental_parity(ours, ref):
    assert len(ours) == len(ref) == 160
    changed_sel = 0
    for step, ((sl, sel), (sr, ref_sel)) in enumerate(zip(ours, ref)):
        assert np.max(np.abs(sl - sr)) < 1e-8, (step, np.max(np.abs(sl - sr)))
        assert np.array_equal(sel, ref_sel), step
        changed_sel += int(np.sum(ref_sel == 1))
    assert changed_sel > 0


def test_incremental_parity_with_reference(lib, incremental_reference):
    """growth in the style of test_gpu_parity._random_growth: loop closures and injected outliers as max factors, on the library
    (native) and on the reference (checker factor): states at every step, selections of the new factors"""
    _incremental_parity(_incremental_ours(lib), incremental_reference)


@pytest.mark.parametrize("opts", INC_FORMS, ids=_ids)
def test_incremental_parity_with_reference_under_every_launch_form(lib, incremental_reference, opts):
    with lib.options(**opts):
        ours = _incremental_ours(lib)
    _incremental_parity(ours, incremental_reference)


def test_foreign_tag3_keeps_host_path(lib, helper):
    """the checker factor with type tag 3 on the PRODUCT library is not native (its eval is not the library's): host path, -4 from
    the resident API, and the same result as native max factors"""
    states, base, loops, outl = mm.m3500_outliers()
    edges = loops[:300] + outl[:10]
    rec = []
    gf = mm.build(lib, states, base, edges, True, mm.helper_adder(lib, helper, 3, rec))
    gn = mm.build(lib, states, base, edges, True)
    pf, pn = lib.new_param(), lib.new_param()
    assert lib.dll.aprilsam_amd_resident_begin(gf.ptr, pf.ptr) == -4
    for _ in range(3):
        gf.cholesky(pf); gn.cholesky(pn)
        assert np.max(np.abs(gf.states() - gn.states())) < 1e-9
        assert np.array_equal(gn.max_selected(pn)[len(base[0]):], [helper.mm_last(f) for f in rec])
    assert np.all(gf.max_selected(pf) == -1)          # (not a native max factor)
    for p in (pf, pn):
        p.destroy()
    gf.destroy(); gn.destroy()


def test_component_edit_seen_by_next_call(lib):
    states, base, loops, outl = mm.m3500_outliers()
    edges = loops[:400]
    g = mm.build(lib, states, base, edges, True)
    p = lib.new_param()
    for _ in range(3):                   # warm: speculative calls and graph replay from here on
        g.cholesky(p)
    st0 = g.states().copy()
    nb = len(base[0])
    fidx = nb + 7
    comp = abi.max_view(C.pointer(g.factor(fidx))).factors[0].contents
    for k in range(3):
        comp.u.z[k] += 0.5                # an in-place edit of the inlier component
    c_edit = g.chi2()
    g.cholesky(p)
    st_edit = g.states()
    # the same graph built from the same states with and without the edit, one step each (a cold plan: same numbers to rounding)
    edges2 = list(edges); a, b, zz, WW = edges2[7]; edges2[7] = (a, b, zz + 0.5, WW)
    out = []
    for e in (edges2, edges):
        g2 = mm.build(lib, st0, base, e, True)
        p2 = lib.new_param()
        out.append((g2.chi2(), None))
        g2.cholesky(p2)
        out[-1] = (out[-1][0], g2.states())
        p2.destroy(); g2.destroy()
    assert abs(out[0][0] - c_edit) <= 1e-12 * c_edit and abs(out[1][0] - c_edit) > 1e-6 * c_edit
    assert np.max(np.abs(st_edit - out[0][1])) < 1e-9
    assert np.max(np.abs(st_edit - out[1][1])) > 1e-6
    p.destroy(); g.destroy()


def test_refusals(lib, tmp_path):
    states, base, loops, outl = mm.m3500_outliers()
    g = mm.build(lib, states, base, loops[:50], True)
    p = lib.new_param()
    d = lib.dll
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    st0 = g.states().copy()
    assert d.aprilsam_amd_shard_begin(C.cast(g.ptr, C.c_void_p), C.cast(p.ptr, C.c_void_p), 0, 1) == -12
    _same(st0, g.states())
    assert not g.save(str(tmp_path / "m.graph"))
    # bad K / asymmetric W: NULL from the constructor, nothing added
    with pytest.raises(ValueError):
        g.make_factor_max(0, 5, np.zeros((9, 3)), np.tile(np.eye(3).reshape(9), (9, 1)), np.zeros(9))
    Wa = np.eye(3).reshape(9).copy(); Wa[1] = 0.3
    with pytest.raises(ValueError):
        g.make_factor_max(0, 5, np.zeros((2, 3)), [np.eye(3).reshape(9), Wa], np.zeros(2))
    # a component edited into an asymmetric W after construction: -12 at the next call, states untouched
    comp = abi.max_view(C.pointer(g.factor(len(base[0]) + 3))).factors[1].contents
    comp.u.W.contents.data[1] = 1e-9
    lib.clear_error()
    g.cholesky(p)
    assert lib.last_error()[0] == -12
    _same(st0, g.states())
    with pytest.raises(RuntimeError):
        g.max_selected(p, [g.n_factors])
    p.destroy(); g.destroy()


# ---- a table move with device-written selections in flight --------------------------------------------------------------------
def test_selections_survive_a_move_of_the_table(lib):
    """tests/support/table_move.py: 140 max factors (K = 2) appended one or two per incremental step, 6 of them before the first batch
    step and a second batch step at the 56th.  The component table moves whenever one of its buffers runs out of room (the capacities
    are worked out in that file: under the rule of commit 362a7eb at 9, 13, 19, 28, 42, 63 and 94 factors, under the robust table's rule
    at 41 and 73), and every selection k_select_mixture wrote must come through: aprilsam_amd_max_selected before and after every
    fast-path step agrees for every older factor.  The steps that take the count past each of those capacities are fast-path steps, and
    so are at least 90 % of all steps (a re-planned step selects everything again and proves nothing).  Checked on a scratch copy: with
    the read-back before the move deleted, this test fails (the first batch step's selections come back as -1)."""
    from tests.support import table_move as tm
    r = tm.grow(lib, tm.scene(3), lambda g, a, b, z, W: g.add_factor_max(a, b, *mm.two_component(z, W)), lambda g, p, idx: g.max_selected(p, idx))
    print(f"max factors {r['family']}, incremental steps {r['steps']}, fast path {r['fast']}, (step, factor) pairs compared {r['checked']}")
    assert r["family"] >= tm.FAMILY_FACTORS_MIN and r["fast"] >= 0.9 * r["steps"]
    for cap in tm.ROW_CAPS["max"]:
        assert any(lo <= cap < hi for lo, hi in r["spans"]), (cap, r["spans"])
    assert set(r["values"].tolist()) == {0, 1}                              # both components won somewhere
