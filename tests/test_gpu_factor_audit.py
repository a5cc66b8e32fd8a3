"""aprilsam_amd_factor_audit (aprilsam_amd/csrc/audit.hip.h): per factor of the system the last solver call
factorised its share of the linear cost, its leverage, its leave-one-out distance and its checkability, against the dense numpy model of
tests/support/audit_model.py (pinned on the CPU by tests/test_audit_model.py), against the two identities that need no tolerance of
their own, for every factor family, behind every kernel path, and the call's contract.

Tolerances (audit_model.tolerances): the project's SIG_RTOL = 1e-9 of row_scale(Sigma) pushed through the formulas to first order --
leverage and checkability absolute SIG_RTOL * row_scale * sum |J' W J| (times 3 for the determinant), d2_loo that bound divided by the
model's det M, relative to max(d2_loo, chi2), compared only where the model's checkability is >= 1e-3; chi2 1e-12 relative (no Sigma in
it).  The step Delta the model audits with is the library's own delta_X: what is compared is the audit, not the solve."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import abi, datasets
from tests.support import audit_model as am
from tests.support import fixed_model, maxmix_model, polar_model, robust_model
from tests.support.consumer_graphs import two_components
from tests.support.kernel_paths import KERNEL_PATHS
from tests.support.marginal_cases import case_arrays, factor_pairs
from tests.support.sigma_compare import SIG_RTOL

pytestmark = pytest.mark.gpu
SENTINEL = -777.25


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _arrays(lib, name):
    return two_components()[0] if name == "two_components" else case_arrays(lib, name)


def _solved(lib, arr, steps=1):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    for _ in range(steps):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
    return g, p


def _model(g, p, arr, fixed=(), W=None):
    """the dense model of the system the last step factorised: at the graph's l_points, with the library's own step"""
    states, fa, fb, z, W0 = arr
    return am.graph_model(g.l_points(), fa, fb, z, W0 if W is None else W, p.c.tikhanov, Delta=g.deltas(), fixed=fixed)


def _raw(lib, g, p, idx, out, n=None):
    ip = None if idx is None else np.ascontiguousarray(idx, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    return lib.dll.aprilsam_amd_factor_audit(g.ptr if g is not None else None, p.ptr if p is not None else None,
                                             (0 if idx is None else len(idx)) if n is None else n, ip,
                                             None if out is None else out.ctypes.data_as(C.POINTER(C.c_double)))


def _library_trace_miss(g, p, rows, lam_nodes=None, n_free=None):
    """the trace identity from the library's own outputs: sum leverage + sum_i lambda_i tr(Sigma_ii) - 3 (free nodes)"""
    d = g.marginals(p)
    N = len(d)
    lam = np.zeros(N); lam[:N if lam_nodes is None else lam_nodes] = p.c.tikhanov
    return am.trace_identity(rows, d, lam, N if n_free is None else n_free)


# ---- 1. against the dense model --------------------------------------------------------------------------------------------------
CASES = ["tutorial", "random0", "random1", "random2", "lattice12", "two_components"]


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_against_the_dense_model(lib, name, steps):
    """every factor (factors == NULL), then a shuffled subset with duplicates; and the trace identity from the library's own outputs"""
    arr = _arrays(lib, name)
    g, p = _solved(lib, arr, steps)
    rows, unaud = g.factor_audit(p)
    assert unaud == 0 and rows.shape == (len(arr[1]), 4)
    model, tol, Sig, facs = _model(g, p, arr)
    worst, below = am.compare(rows, model, tol)
    print(f"[audit] {name} after {steps}: worst error / tolerance (chi2, leverage, d2_loo, checkability) {worst}; {below} of {len(rows)} factors "
          f"below the checkability floor")
    if name in ("random1", "random2"):
        # (the floor leaves out 7 of 140 and 16 of 750 at the goldens' initial states -- the system of the first step; re-counted here at the
        # state each run solved to)
        assert below <= 0.1 * len(rows), (below, len(rows))
    assert np.all(rows[:, 1] >= -tol[:, 1]) and np.all(rows[:, 1] <= 3 + tol[:, 1])
    assert np.all(rows[:, 3] >= -tol[:, 3]) and np.all(rows[:, 3] <= 1 + tol[:, 3])
    rng = np.random.default_rng(len(rows))
    idx = rng.integers(0, len(rows), max(4, len(rows) // 2)).astype(np.int32)
    idx[1] = idx[0]                                              # (a duplicate for sure)
    sub, unaud = g.factor_audit(p, idx)
    assert unaud == 0 and sub.tobytes() == rows[idx].tobytes()
    N = len(arr[0])
    miss = _library_trace_miss(g, p, rows)
    print(f"[audit] {name} after {steps}: trace identity miss {miss:.3e} (bound {SIG_RTOL * 3 * N:.1e})")
    assert abs(miss) <= SIG_RTOL * 3 * N, miss
    p.destroy(); g.destroy()


@pytest.mark.parametrize("name", ["random2", "lattice12"])
def test_both_block_locations_occur(lib, name):
    """k_factor_audit finds a factor's block in the front of its earlier-eliminated node: the other node among that front's own rows, or
    among its struct rows (binary search).  Both occur in the graphs above, in both orientations of (a, b), and the prior's 3 x 3 block"""
    from tests.support.mf_emulator import PlanView
    states, fa, fb, z, W = _arrays(lib, name)
    P = PlanView(lib, len(states), fa, fb, xy=states[:, :2])
    pos_front = np.zeros(P.N, np.int64)
    for t in range(P.nF):
        pos_front[P.front_first[t]:P.front_first[t] + P.front_nsb[t]] = t
    a, b = factor_pairs(fa, fb)
    qa, qb = P.pos[a], P.pos[b]
    t = pos_front[np.minimum(qa, qb)]
    later = np.maximum(qa, qb)
    own = (later >= P.front_first[t]) & (later < P.front_first[t] + P.front_nsb[t])
    assert own.any() and (~own).any()
    assert (qa < qb).any() and (qa > qb).any() and (np.asarray(fb) < 0).any()
    for k in np.nonzero(~own)[0][:50]:                           # (a struct row is where the plan says it is)
        rw = P.front_rows[P.front_rows_ptr[t[k]]:P.front_rows_ptr[t[k] + 1]]
        assert later[k] in rw


# ---- 2. the trace identity at M3500's size, and rows recomputed from marginals_joint's blocks ----------------------------------------
def test_m3500_trace_identity_and_rows_from_joint_blocks(lib):
    arr = datasets.m3500_batch()
    states, fa, fb, z, W = arr
    g, p = _solved(lib, arr, 5)
    rows, unaud = g.factor_audit(p)
    assert unaud == 0 and len(rows) == len(fa) and np.isfinite(rows[:, [0, 1, 3]]).all()
    N = len(states)
    miss = _library_trace_miss(g, p, rows)
    print(f"[audit] m3500: {len(rows)} factors, trace identity miss {miss:.3e} (bound {SIG_RTOL * 3 * N:.1e})")
    assert abs(miss) <= SIG_RTOL * 3 * N, miss
    lp, dx = g.l_points(), g.deltas()
    pick = np.random.default_rng(3500).choice(len(fa), 50, replace=False)
    pick[0] = int(np.nonzero(fb < 0)[0][0])                      # (the prior among them)
    facs = am.xyt_factors(lp, fa[pick], fb[pick], z[pick], W[pick])
    for k, f in enumerate(pick):
        a, b = int(fa[f]), int(fb[f])
        Sff = g.marginals(p, [a])[0] if b < 0 else g.marginals_joint(p, [a], [b])[0]
        want = am.one(Sff, dx[a] if b < 0 else np.r_[dx[a], dx[b]], facs[k])
        fac = facs[k]
        J = fac[2] if fac[3] is None else np.hstack([fac[2], fac[3]])
        lev = SIG_RTOL * np.abs(Sff).max() * np.abs(J.T @ fac[5] @ J).sum()      # (the block's own largest entry: no larger than the row scale)
        assert abs(rows[f, 0] - want[0]) <= am.CHI2_RTOL * abs(want[0]), (f, rows[f], want)
        assert abs(rows[f, 1] - want[1]) <= lev and abs(rows[f, 3] - want[3]) <= 3 * lev, (f, rows[f], want, lev)
        if want[3] >= am.CHECK_FLOOR:
            assert abs(rows[f, 2] - want[2]) <= lev / want[3] * max(want[2], want[0]), (f, rows[f], want)
    p.destroy(); g.destroy()


# ---- 3. leave one out for real ---------------------------------------------------------------------------------------------------
def test_leave_one_out_for_real(lib):
    """random_1: the factor with the largest checkability is taken out, the reduced graph solved from the same states (so the same
    l_points), and the factor gated in numpy against that param's joint block and step: e' S^-1 e is the full graph's d2_loo"""
    arr = case_arrays(lib, "random1")
    states, fa, fb, z, W = arr
    g, p = _solved(lib, arr)
    rows, _ = g.factor_audit(p)
    model, tol, Sig, facs = _model(g, p, arr)
    bi = np.nonzero(fb >= 0)[0]
    f = int(bi[np.argmax(rows[bi, 3])])
    keep = np.arange(len(fa)) != f
    arr2 = (states, fa[keep], fb[keep], z[keep], W[keep])
    g2, p2 = _solved(lib, arr2)
    assert g2.l_points().tobytes() == g.l_points().tobytes()
    a, b, Ja, Jb, r, Wf = facs[f]
    J = np.hstack([Ja, Jb])
    d = g2.deltas()
    e = r - J @ np.r_[d[a], d[b]]
    S = J @ g2.marginals_joint_any(p2, [a], [b])[0] @ J.T + np.linalg.inv(Wf)
    loo = float(e @ np.linalg.solve(S, e))
    print(f"[audit] leave-one-out: factor {f} ({a}, {b}) checkability {rows[f, 3]:.4f}: d2_loo {rows[f, 2]:.15g}, reduced graph {loo:.15g}")
    assert abs(loo - rows[f, 2]) <= tol[f, 2] * max(rows[f, 2], rows[f, 0]), (loo, rows[f], tol[f])
    for x in (p, g, p2, g2):
        x.destroy()


# ---- 4. every factor family ------------------------------------------------------------------------------------------------------
def test_robust_factors_are_audited_with_their_weight(lib):
    """Cauchy on the closures of random_1: the slot holds W_eff = w W, w as aprilsam_amd_robust_weights reports it"""
    arr = case_arrays(lib, "random1")
    states, fa, fb, z, W = arr
    closure = (fb >= 0) & (np.abs(fa - fb) > 1)
    kinds = np.where(closure, robust_model.CAUCHY, robust_model.NONE); cs = np.where(closure, 1.0, 0.0)
    g = robust_model.build(lib, states, (fa, fb, z, W), kinds, cs); p = lib.new_param()
    for _ in range(2):
        g.cholesky(p)
    w = g.robust_weights(p)
    assert (w[closure] > 0).all() and (w[closure] < 1).any() and (w[~closure] == -1).all()
    Weff = np.where(closure, w, 1.0)[:, None] * np.asarray(W, float).reshape(-1, 9)
    rows, unaud = g.factor_audit(p)
    model, tol, _, _ = _model(g, p, arr, W=Weff)
    worst, below = am.compare(rows, model, tol)
    print(f"[audit] robust: worst {worst}, {below} below the floor")
    assert unaud == 0
    p.destroy(); g.destroy()


def test_max_mixtures_are_audited_with_the_selected_component(lib):
    arr = case_arrays(lib, "random1")
    states, fa, fb, z, W = arr
    closure = (fb >= 0) & (np.abs(fa - fb) > 1)
    base = (fa[~closure], fb[~closure], z[~closure], W[~closure])
    edges = [(int(fa[i]), int(fb[i]), z[i], W[i]) for i in np.nonzero(closure)[0]]
    edges[0] = (edges[0][0], edges[0][1], edges[0][2] + np.array([3.0, -3.0, 1.0]), edges[0][3])      # (one that selects the null hypothesis)
    g = maxmix_model.build(lib, states, base, edges, as_max=True); p = lib.new_param()
    g.cholesky(p)
    sel = g.max_selected(p)
    nb = len(base[0])
    assert (sel[:nb] == -1).all() and sel[nb] == 1 and (sel[nb + 1:] == 0).any()
    za = np.vstack([base[2], np.array([e[2] for e in edges])])
    Wa = np.vstack([np.asarray(base[3], float).reshape(-1, 9),
                    np.array([maxmix_model.two_component(e[2], e[3])[1][sel[nb + k]] for k, e in enumerate(edges)])])
    arr2 = (states, np.r_[base[0], [e[0] for e in edges]].astype(np.int32), np.r_[base[1], [e[1] for e in edges]].astype(np.int32), za, Wa)
    rows, unaud = g.factor_audit(p)
    model, tol, _, _ = _model(g, p, arr2)
    worst, below = am.compare(rows, model, tol)
    print(f"[audit] max-mixture: worst {worst}, {below} below the floor")
    assert unaud == 0
    p.destroy(); g.destroy()


def test_polar_factors_are_audited_in_their_xyt_slot(lib):
    """range, bearing and range-bearing factors on a graph with landmark nodes.  The library audits the SLOT, so its rows are held to the
    model of the slot it reads -- xyt_factors on (z_eff, W_eff) of aprilsam_amd_debug_polar_slot, the residual taken as z_eff - q like the
    kernel's -- with chi2 to 1e-12 relative, and leverage <= rank W + bound.  That the slot form IS the true 1- or 2-row factor (chi2 =
    r_p' W_p r_p of the polar residual minus its linear correction) is a separate statement about two numpy models, and only that one
    carries what storing the slot as a measurement costs (audit_model.polar_chi2_allowance)"""
    sc = polar_model.snake(5, 4, seed=2)
    plain, polars = sc["plain"], sc["polars"]
    assert {pol[0] for pol in polars} == {polar_model.RANGE, polar_model.BEARING, polar_model.RANGE_BEARING}
    g = polar_model.build(lib, sc["start"], plain, polars); p = lib.new_param()
    for _ in range(2):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
    lp, dx = g.l_points(), g.deltas()
    nP = len(plain[0])
    slots = [lib.polar_slot(pol[0], lp[pol[1]], lp[pol[2]], pol[3], pol[4]) for pol in polars]
    facs = am.xyt_factors(lp, *plain) + am.xyt_factors(lp, np.array([pol[1] for pol in polars]), np.array([pol[2] for pol in polars]),
                                                       np.array([ze for ze, We in slots]), np.array([We for ze, We in slots]))
    Sig = np.linalg.inv(am.dense_A(lp, facs, p.c.tikhanov))
    model = am.audit(Sig, dx, facs)
    tol = am.tolerances(Sig, facs, model)
    rows, unaud = g.factor_audit(p)
    assert unaud == 0
    print("[audit] polar: chi2 error / chi2 against the slot's model", np.abs(rows[nP:, 0] - model[nP:, 0]) / model[nP:, 0])
    worst, below = am.compare(rows, model, tol)
    print(f"[audit] polar: worst {worst}, {below} below the floor")
    true = am.audit(Sig, dx, am.polar_factors(lp, polars))       # (the m-row factors: the same Sigma, J_eff' W_eff J_eff = J_p' W_p J_p)
    for k, pol in enumerate(polars):
        m = polar_model.rows(pol[0])
        assert rows[nP + k, 1] <= m + tol[nP + k, 1], (pol[0], rows[nP + k])
        Ja, Jb, r, Wp = polar_model.evaluate(lp, pol)
        v = r - Ja @ dx[pol[1]] - Jb @ dx[pol[2]]
        chi2_p = float(v @ Wp @ v)
        allow = am.polar_chi2_allowance(chi2_p, *slots[k])
        assert abs(model[nP + k, 0] - chi2_p) <= am.CHI2_RTOL * chi2_p + allow, (pol[0], model[nP + k, 0], chi2_p, allow)
        assert abs(model[nP + k, 1] - true[k, 1]) <= tol[nP + k, 1] and abs(model[nP + k, 3] - true[k, 3]) <= tol[nP + k, 3], (pol[0], model[nP + k], true[k])
    p.destroy(); g.destroy()


@pytest.mark.parametrize("fixed", fixed_model.FIXED_SETS, ids=str)
def test_fixed_nodes(lib, fixed):
    sc = fixed_model.chain8()
    fa, fb, z, W = sc["plain"]
    g = fixed_model.build(lib, sc["start"], sc["plain"], fixed=fixed); p = lib.new_param()
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    arr = (sc["start"], fa, fb, z, W)
    rows, unaud = g.factor_audit(p)
    model, tol, _, _ = _model(g, p, arr, fixed=fixed)
    worst, below = am.compare(rows, model, tol)
    N = len(sc["start"])
    miss = _library_trace_miss(g, p, rows, n_free=N - len(fixed))
    assert unaud == 0 and abs(miss) <= SIG_RTOL * 3 * N, miss
    seen = 0
    for f, (a, b) in enumerate(zip(fa, fb)):                     # all of a factor's nodes fixed: P = 0 exactly
        if a in fixed and (b < 0 or b in fixed):
            assert rows[f, 1] == 0.0 and rows[f, 3] == 1.0 and rows[f, 2] == rows[f, 0], rows[f]
            seen += 1
    assert seen == (1 if fixed in ((2, 3), (5,)) else 0)
    p.destroy(); g.destroy()


def test_host_evaluated_factors_are_counted_and_nan(lib, tmp_path):
    from tests.support import custom_scenario
    cl = custom_scenario.build_custom_lib(str(tmp_path))
    states, fa, fb, z, W = datasets.random_pose_graph(40, 25, seed=5)
    g = lib.new_graph(); g.build_from_arrays(states, fa, fb, z, W); p = lib.new_param()
    nat = len(fa)
    Wm = np.array([40.0, 3.0, 3.0, 50.0])
    for a, b in ((3, 17), (20, 8)):
        lib._add_factor(g.ptr, cl.custom_xy_create(a, b, (C.c_double * 2)(0.5, -0.25), (C.c_double * 4)(*Wm)))
    lib._add_factor(g.ptr, cl.custom_midpoint_create(5, 11, 30, (C.c_double * 2)(0.1, 0.2), (C.c_double * 4)(*Wm)))
    g.add_factor_xyt(0, 39, [0.3, 0.1, 0.0], np.eye(3) * 50)      # (a native factor behind them)
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    rows, unaud = g.factor_audit(p)
    assert unaud == 3 and np.isnan(rows[nat:nat + 3]).all() and np.isfinite(rows[:nat, [0, 1, 3]]).all() and np.isfinite(rows[nat + 3, [0, 1, 3]]).all()
    native = np.r_[np.arange(nat), nat + 3].astype(np.int32)
    only, unaud = g.factor_audit(p, native)
    assert unaud == 0 and only.tobytes() == rows[native].tobytes()
    mixed, unaud = g.factor_audit(p, [nat + 2, 0, nat, nat])
    assert unaud == 3 and np.isnan(mixed[[0, 2, 3]]).all() and mixed[1].tobytes() == rows[0].tobytes()
    p.destroy(); g.destroy()


# ---- 5. kernel paths and the resident loops ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", KERNEL_PATHS, ids=_ids)
def test_behind_every_kernel_path(lib, opts):
    arr = case_arrays(lib, "random1")
    with lib.options(**opts):
        g, p = _solved(lib, arr, 2)
        rows, unaud = g.factor_audit(p)
        model, tol, _, _ = _model(g, p, arr)
        p.destroy(); g.destroy()
    am.compare(rows, model, tol)
    assert unaud == 0


@pytest.mark.parametrize("how", ["batch_resident", "begin_steps_end"])
def test_after_resident_loops(lib, how):
    """the factor of the LAST iteration, at the l_points resident_end leaves in the node objects, with that iteration's delta_X"""
    arr = case_arrays(lib, "random1")
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    d = lib.dll
    if how == "batch_resident":
        g.batch_resident(p, 3)
    else:
        assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
        assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 3, 0) == 0
        out = np.full((len(arr[1]), 4), SENTINEL)
        assert _raw(lib, g, p, None, out) == -1 and (out == SENTINEL).all()      # during a resident run: no retained factor
        assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
        assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    assert np.max(np.abs(g.l_points() - arr[0])) > 1e-6
    rows, unaud = g.factor_audit(p)
    model, tol, _, _ = _model(g, p, arr)
    am.compare(rows, model, tol)
    assert unaud == 0
    p.destroy(); g.destroy()


def test_after_an_incremental_call_that_fell_back_to_a_batch_step(lib):
    """option inc_fast = 0: april_graph_cholesky_inc re-plans and factorises everything -- the xyt factors at the nodes' l_points, the
    priors at the points they entered at (the batch step's linearisation point), lambda on the nodes of the last batch step.  The prior's
    node is re-linearised before the call, so the two points differ and a prior audited at the wrong one misses chi2 and d2_loo; the whole
    audit is compared with the dense model of exactly that system, and the trace identity holds from the library's own outputs"""
    arr = case_arrays(lib, "random1")
    states, fa, fb, z, W = arr
    g, p = _solved(lib, arr)
    N = g.n_nodes
    entered = g.l_points()                                       # (where the batch step linearised: the priors' points from now on)
    prior = np.nonzero(fb < 0)[0]
    for a in fa[prior]:
        g.set_state(int(a), g.states_of(int(a)), relinearize=True)
    last = np.array(g.states_of(N - 1))
    g.add_node_xyt(last + np.array([1.0, 0.1, 0.05]))
    new = [(N - 1, N, [1.0, 0.0, 0.05], np.diag([100.0, 100.0, 400.0])), (3, N, [0.2, 0.1, 0.0], np.diag([10.0, 10.0, 40.0]))]
    for a, b, zz, WW in new:
        g.add_factor_xyt(a, b, zz, WW)
    p.c.batch_time = 1e300
    with lib.options(inc_fast=0):
        g.cholesky_inc(p)
    assert p.stats()["inc_replanned"] == 1 and p.stats()["not_spd"] == 0
    rows, unaud = g.factor_audit(p)
    assert unaud == 0 and len(rows) == len(fa) + 2 and np.isfinite(rows[:, [0, 1, 3]]).all()
    miss = _library_trace_miss(g, p, rows, lam_nodes=N)
    assert abs(miss) <= SIG_RTOL * 3 * (N + 1), miss
    lp, dx = g.l_points(), g.deltas()
    assert len(prior) and all(np.abs(lp[a] - entered[a]).max() > 1e-6 for a in fa[prior])
    fa2 = np.r_[fa, [n[0] for n in new]]; fb2 = np.r_[fb, [n[1] for n in new]]
    z2 = np.vstack([z, [n[2] for n in new]]); W2 = np.vstack([np.asarray(W, float).reshape(-1, 9), [n[3].ravel() for n in new]])
    facs = am.xyt_factors(lp, fa2, fb2, z2, W2)
    at_entry = am.xyt_factors(entered, fa[prior], fb[prior], z[prior], W[prior])
    for k, f in enumerate(prior):
        facs[f] = at_entry[k]
    A = am.dense_A(lp, facs, 0.0)
    A[:3 * N, :3 * N] += p.c.tikhanov * np.eye(3 * N)
    Sig = np.linalg.inv(A)
    model = am.audit(Sig, dx, facs)
    worst, below = am.compare(rows, model, am.tolerances(Sig, facs, model))
    wrong = am.audit(Sig, dx, am.xyt_factors(lp, fa[prior], fb[prior], z[prior], W[prior]))
    print(f"[audit] incremental fallback: worst {worst}; priors' chi2 {rows[prior, 0]}, at the nodes' l_points it would be {wrong[:, 0]}")
    assert all(abs(wrong[k, 0] - model[f, 0]) > 1e-6 * model[f, 0] for k, f in enumerate(prior))      # (the two points tell apart)
    p.destroy(); g.destroy()


# ---- 6. the contract -------------------------------------------------------------------------------------------------------------
def test_same_bits_and_one_selected_inversion(lib):
    arr = case_arrays(lib, "random2")
    g, p = _solved(lib, arr, 2)
    runs = lambda: lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    r0 = runs()
    a, _ = g.factor_audit(p)
    assert runs() == r0 + 1
    b, _ = g.factor_audit(p)
    m = g.marginals(p)
    c, _ = g.factor_audit(p, np.arange(len(a), dtype=np.int32))
    assert runs() == r0 + 1 and a.tobytes() == b.tobytes() == c.tobytes()
    g.cholesky(p)
    g.factor_audit(p)
    assert runs() == r0 + 2
    assert m.shape == (len(arr[0]), 3, 3)
    p.destroy(); g.destroy()


def test_batch_and_resident_steps_are_bitwise_unaffected(lib):
    arr = case_arrays(lib, "random2")
    runs = []
    for with_audit in (False, True):
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        snaps = []
        for k in range(6):
            if k < 4:
                g.cholesky(p)
            else:
                g.batch_resident(p, 2)
            if with_audit:
                g.factor_audit(p); g.factor_audit(p, [0, 5, 5])
            snaps.append(np.concatenate([g.states(), g.deltas(), g.l_points()]).tobytes())
        runs.append(snaps)
        p.destroy(); g.destroy()
    assert runs[0] == runs[1]


def test_params_on_two_slots(lib):
    arr = case_arrays(lib, "lattice12")
    out = []
    for slots in ((0, 0), (0, 1)):
        gs, ps = [], []
        for s in slots:
            g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
            assert lib.dll.aprilsam_amd_param_set_device(p.ptr, s) == 0
            g.cholesky(p); gs.append(g); ps.append(p)
        a = [g.factor_audit(p)[0] for g, p in zip(gs, ps)]
        for g, p in zip(gs, ps):
            g.cholesky(p)
        out.append([a[0].tobytes(), a[1].tobytes()] + [g.states().tobytes() for g in gs])
        for x in gs + ps:
            x.destroy()
    assert out[0][0] == out[0][1] == out[1][0] == out[1][1]
    assert out[0][2:] == out[1][2:]


def test_two_params_on_one_graph(lib):
    """lp, Delta and the weighted slots live with the graph, shared by every param that solves it: after another param's solver call the
    first param's factor is still retained (marginals answers) but the pack no longer holds what it linearised -- refused with -1, nothing
    written, until that param's next batch call; april_graph_chi2 in between linearises nothing and ends nothing"""
    arr = case_arrays(lib, "random1")
    g = lib.new_graph(); g.build_from_arrays(*arr); pa = lib.new_param(); pb = lib.new_param()
    g.cholesky(pa)
    rows_a, _ = g.factor_audit(pa)
    g.chi2()
    assert g.factor_audit(pa)[0].tobytes() == rows_a.tobytes()
    g.cholesky(pb)                                               # (linearises at the states pa's step moved to)
    rows_b, _ = g.factor_audit(pb)
    model, tol, _, _ = _model(g, pb, arr)
    am.compare(rows_b, model, tol)
    assert rows_b.tobytes() != rows_a.tobytes()
    assert g.marginals(pa).shape == (len(arr[0]), 3, 3)           # pa's factor and Sigma are still there
    msg = _refused(lib, g, pa, None, -1)
    assert "another" in msg
    _refused(lib, g, pa, [0, 1], -1)
    assert g.factor_audit(pb)[0].tobytes() == rows_b.tobytes()     # (the refusal disturbed nothing of pb's)
    g.cholesky(pa)                                               # pa's next batch call: available again, and right
    ra, _ = g.factor_audit(pa)
    model, tol, _, _ = _model(g, pa, arr)
    am.compare(ra, model, tol)
    g.optimize_lm(pb, max_iters=2)                               # an LM run of the other param: the same refusal
    assert g.marginals(pa).shape == (len(arr[0]), 3, 3)
    _refused(lib, g, pa, None, -1)
    _next_step_succeeds(lib, g, pa)
    for x in (pa, pb, g):
        x.destroy()


def _refused(lib, g, p, idx, code, n=None, out_rows=None):
    """the call returns `code`, leaves the sentinel in `out` and sets the last error"""
    rows = out_rows if out_rows is not None else (g.n_factors if g is not None else 4)
    out = np.full((max(rows, 1), 4), SENTINEL)
    lib.clear_error()
    rc = _raw(lib, g, p, idx, out, n)
    assert rc == code, (rc, code, lib.last_error())
    assert (out == SENTINEL).all()
    assert lib.last_error()[0] == code, lib.last_error()
    return lib.last_error()[1]


def _next_step_succeeds(lib, g, p):
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0 and p.stats()["error_code"] == 0
    rows, unaud = g.factor_audit(p)
    assert np.isfinite(rows[:, [0, 1, 3]]).all()


def test_refusals_leave_everything_in_place(lib):
    arr = case_arrays(lib, "random1")
    F = len(arr[1])
    ref_g, ref_p = _solved(lib, arr, 2)
    ref_rows, _ = ref_g.factor_audit(ref_p)
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    _refused(lib, g, p, None, -1)                                # never solved
    g.cholesky(p)
    _refused(lib, g, p, [0, F], -13)                             # a factor index out of range
    _refused(lib, g, p, [-1], -13)
    _refused(lib, g, p, [0], -13, n=-1)                          # n < 0
    _refused(lib, None, p, [0], -13)                             # null arguments
    _refused(lib, g, None, [0], -13)
    lib.clear_error()
    assert _raw(lib, g, p, [0], None) == -13 and lib.last_error()[0] == -13
    g.cholesky(p)                                                # the next solver call: the bits of the undisturbed run
    assert g.states().tobytes() == ref_g.states().tobytes()
    assert g.factor_audit(p)[0].tobytes() == ref_rows.tobytes()
    # factors added since: outside the factors that call packed; NULL lists the factorised system's factors only
    g.add_factor_xyt(0, 7, [0.1, 0.2, 0.0], np.eye(3) * 10)
    _refused(lib, g, p, [F], -13)
    part, _ = g.factor_audit(p)
    assert part.shape == (F + 1, 4) and part[:F].tobytes() == ref_rows.tobytes() and np.isnan(part[F]).all()
    # nodes added since: the node count differs
    n = g.n_nodes
    g.add_node_xyt([0.5, 0.5, 0.0]); g.add_factor_xyt(n - 1, n, [0.1, 0, 0], np.eye(3) * 10)
    _refused(lib, g, p, [0], -13)
    _next_step_succeeds(lib, g, p)
    for x in (p, g, ref_p, ref_g):
        x.destroy()


def test_refused_without_a_factor_of_the_right_kind(lib):
    arr = case_arrays(lib, "random1")
    d = lib.dll
    # after optimize_lm, initialize_chordal and optimize_gnc: they drop the retained factor
    g, p = _solved(lib, arr)
    g.optimize_lm(p, max_iters=3)
    _refused(lib, g, p, None, -1)
    _next_step_succeeds(lib, g, p)
    g.initialize_chordal(p)
    _refused(lib, g, p, None, -1)
    _next_step_succeeds(lib, g, p)
    g.optimize_gnc(p, np.nonzero((arr[2] >= 0) & (np.abs(arr[1] - arr[2]) > 1))[0].astype(np.int32), max_iters=3, max_stages=2)
    _refused(lib, g, p, None, -1)
    _next_step_succeeds(lib, g, p)
    # sharded param
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    d.aprilsam_amd_shard_end.argtypes = [C.c_void_p]
    assert d.aprilsam_amd_shard_begin(C.cast(g.ptr, C.c_void_p), C.cast(p.ptr, C.c_void_p), 0, 1) == 0
    _refused(lib, g, p, None, -12)
    d.aprilsam_amd_shard_end(C.cast(p.ptr, C.c_void_p))
    _next_step_succeeds(lib, g, p)
    # a fast incremental step: the extended structure (a param's first incremental call re-plans, with room for the steps that follow: after
    # that one the audit answers; the next step takes the fast path)
    p.c.batch_time = 1e300
    fast = False
    for _ in range(3):
        N = g.n_nodes
        g.add_node_xyt(np.array(g.states_of(N - 1)) + np.array([1.0, 0.0, 0.0]))
        g.add_factor_xyt(N - 1, N, [1.0, 0.0, 0.0], np.diag([100.0, 100.0, 400.0]))
        g.cholesky_inc(p)
        assert p.stats()["not_spd"] == 0
        if p.stats()["inc_replanned"] == 0:
            fast = True
            break
        rows, unaud = g.factor_audit(p)
        assert unaud == 0 and len(rows) == g.n_factors and np.isfinite(rows[:, [0, 1, 3]]).all()
    assert fast
    msg = _refused(lib, g, p, None, -12)
    assert "incremental" in msg and "batch" in msg
    with lib.options(batch_extend=0):
        _next_step_succeeds(lib, g, p)
    p.destroy(); g.destroy()
    # asymmetric W in the factorised graph
    from tests.support.asym_scenarios import batch_graph
    ga = lib.new_graph(); ga.build_from_arrays(*batch_graph()); pa = lib.new_param()
    ga.cholesky(pa)
    _refused(lib, ga, pa, None, -12)
    ga.cholesky(pa)
    assert pa.stats()["error_code"] == 0
    pa.destroy(); ga.destroy()
    # the Sigma pool under mem_cap_mb
    gl, pl = _solved(lib, case_arrays(lib, "lattice60"))
    with lib.options(mem_cap_mb=1):
        _refused(lib, gl, pl, [0, 1], -11)
    _next_step_succeeds(lib, gl, pl)
    pl.destroy(); gl.destroy()
