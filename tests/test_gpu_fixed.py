"""Fixed nodes on the GPU: the mask itself (bitwise), one batch step, toggling on a warm param, the resident
loop, every kernel path, every kind of factor that writes a slot before the mask, LM, GNC, the consumers of the retained factor and
every refusal, against the dense numpy model of tests/support/fixed_model.py.  Tolerance: the project's 1e-9, relative to the largest
entry compared (as tests/test_gpu_polar.py)."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import abi, datasets, host
from tests.support import asym_scenarios, custom_scenario, gate_model, lm_model, maxmix_model
from tests.support import fixed_model as fm
from tests.support import gnc_model as gm
from tests.support import polar_model as pm
from tests.support.kernel_paths import KERNEL_PATHS
from tests.support.mf_emulator import PlanView

pytestmark = pytest.mark.gpu
TOL = 1e-9
TIK = pm.TIKHANOV


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(f"{what}: deviation {err:.3e}")
    assert err <= tol, (what, err)
    return err


def _states_close(got, want, what, tol=TOL):
    d = np.asarray(got) - np.asarray(want)
    d[:, 2] = fm.mod2pi(d[:, 2])
    return _close(d, np.zeros_like(d), what, tol * max(1.0, np.abs(want[:, :2]).max()))


def _bits(a):
    return np.ascontiguousarray(a, float).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _stage(lib, g, p):
    """aprilsam_amd_debug_stage what = 1: the assembled (A [3N, 3N], B [3N]) in node coordinates"""
    lib.dll.aprilsam_amd_debug_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    n = 3 * g.n_nodes
    out = np.zeros(n * n + n)
    rc = lib.dll.aprilsam_amd_debug_stage(C.cast(g.ptr, C.c_void_p), C.cast(p.ptr, C.c_void_p), 1, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, (rc, lib.last_error())
    return out[:n * n].reshape(n, n).copy(), out[n * n:].copy()


def _param(lib, tik=None):
    p = lib.new_param()
    assert p.c.tikhanov == TIK
    if tik is not None:
        p.c.tikhanov = tik
    return p


def _fix(g, fixed, on=True):
    for i in fixed:
        assert g.set_fixed(int(i), on) == 0


def _check_fixed_untouched(g, x0, fixed, what):
    st, dx = g.states(), g.deltas()
    for i in fixed:
        assert np.all(dx[i] == 0.0), (what, i, dx[i])                         # +-0 exactly
        assert _same_bits(st[i, :2], x0[i, :2]), (what, i)                    # x and y: bitwise
        assert fm.unchanged_by_wrap(x0[i, 2]) and _same_bits(st[i, 2], x0[i, 2]), (what, i)


@pytest.fixture(scope="module")
def chain():
    d = fm.chain8()
    assert np.all(fm.unchanged_by_wrap(d["start"][:, 2]))                    # the precondition of every "heading bitwise unchanged" below
    return d


# ---- 1. the mask itself, model-free and bitwise --------------------------------------------------------------------------------
@pytest.mark.parametrize("tik", [None, 0.0], ids=["tikhanov=default", "tikhanov=0"])
def test_mask_is_exact(lib, chain, tik):
    g0 = fm.build(lib, chain["start"], chain["plain"]); p0 = _param(lib, tik)
    A0, B0 = _stage(lib, g0, p0)
    lam = TIK if tik is None else tik
    Am, _ = fm.system(chain["start"], chain["plain"], lam=lam)
    _close(A0, Am, "A with nobody fixed against the model")
    for fixed in fm.FIXED_SETS:
        g = fm.build(lib, chain["start"], chain["plain"], fixed=fixed); p = _param(lib, tik)
        A, B = _stage(lib, g, p)
        wantA, wantB = fm.mask(A0, B0, fixed)
        assert _same_bits(A, wantA) and _same_bits(B, wantB), fixed
        idx = fm.dofs(fixed)
        assert np.array_equal(A[np.ix_(idx, idx)], np.eye(len(idx)))          # exactly 1.0 * I: not 1 + tikhanov
        # the same on the param that saw the graph with nobody fixed (its d_lambda cache holds the uniform value) ...
        _fix(g0, fixed)
        A2, B2 = _stage(lib, g0, p0)
        assert _same_bits(A2, wantA) and _same_bits(B2, wantB), fixed
        # ... and back
        _fix(g0, fixed, False)
        A3, B3 = _stage(lib, g0, p0)
        assert _same_bits(A3, A0) and _same_bits(B3, B0), fixed
        p.destroy(); g.destroy()
    p0.destroy(); g0.destroy()


# ---- 2. one batch step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", fm.FIXED_SETS, ids=str)
def test_one_batch_step(lib, chain, fixed):
    x0 = chain["start"]
    g = fm.build(lib, x0, chain["plain"], fixed=fixed); p = _param(lib)
    lib.clear_error()
    g.cholesky(p)
    assert lib.last_error()[0] == 0 and p.stats()["not_spd"] == 0
    A, B = fm.system(x0, chain["plain"], lam=TIK)
    d = fm.reduced_solve(A, B, fixed)
    _close(g.deltas(), d.reshape(-1, 3), f"{fixed}: dx")
    _states_close(g.states(), fm.step(x0, d), f"{fixed}: states")
    _check_fixed_untouched(g, x0, fixed, fixed)
    assert np.array_equal(g.l_points(), x0)
    assert [g.get_fixed(i) for i in range(8)] == [i in fixed for i in range(8)]      # the call leaves the flags alone
    p.destroy(); g.destroy()


def test_fixed_heading_outside_the_range_comes_back_wrapped(lib, chain):
    """the documented rule: a fixed node's heading passes through the state update's mod2pi like any other node's"""
    x0 = chain["start"].copy()
    x0[3, 2] += 2.0 * np.pi                                                  # node 3: fixed, heading outside [-pi, pi)
    x0[5, 2] -= 2.0 * np.pi                                                  # node 5: free, the same the other way
    assert not fm.unchanged_by_wrap(x0[3, 2]) and not -np.pi <= x0[3, 2] < np.pi
    fixed = (0, 3)
    g = fm.build(lib, x0, chain["plain"], fixed=fixed); p = _param(lib)
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    A, B = fm.system(x0, chain["plain"], lam=TIK)
    d = fm.reduced_solve(A, B, fixed)
    want = fm.step(x0, d)
    st, dx = g.states(), g.deltas()
    _close(dx, d.reshape(-1, 3), "dx")
    _close(st, want, "states, wrapped headings included")
    assert np.all(dx[3] == 0.0) and _same_bits(st[3, :2], x0[3, :2])
    assert st[3, 2] == fm.mod2pi(x0[3, 2]) and -np.pi <= st[3, 2] < np.pi      # wrapped like the free node's
    assert -np.pi <= st[5, 2] < np.pi
    _check_fixed_untouched(g, x0, (0,), "node 0")
    p.destroy(); g.destroy()


@pytest.mark.parametrize("with_prior", [True, False], ids=["with the prior", "relative only"])
def test_node_0_fixed_makes_tikhanov_0_regular(lib, chain, with_prior):
    fa, fb, z, W = chain["plain"]
    plain = chain["plain"] if with_prior else tuple(v[fb >= 0] for v in (fa, fb, z, W))
    x0 = chain["start"]
    g = fm.build(lib, x0, plain, fixed=(0,)); p = _param(lib, 0.0)
    lib.clear_error()
    g.cholesky(p)
    assert lib.last_error()[0] == 0 and p.stats()["not_spd"] == 0 and p.stats()["error_code"] == 0
    A, B = fm.system(x0, plain, lam=0.0)
    d = fm.reduced_solve(A, B, (0,))
    _close(g.deltas(), d.reshape(-1, 3), "dx at tikhanov 0")
    _states_close(g.states(), fm.step(x0, d), "states at tikhanov 0")
    _check_fixed_untouched(g, x0, (0,), "node 0")
    p.destroy(); g.destroy()


# ---- 3. toggle on a warm param ---------------------------------------------------------------------------------------------------
def test_toggle_on_a_warm_param(lib, chain):
    topo = ("n_nodes", "n_factors", "n_fronts", "n_levels", "max_front_rows", "nnz_L")
    g = fm.build(lib, chain["start"], chain["plain"]); p = _param(lib)
    for _ in range(3):
        g.cholesky(p)                                                       # cold, warm, replayed
    before = {k: p.stats()[k] for k in topo}
    x3 = g.states()
    _fix(g, (3,))
    g.cholesky(p)
    assert p.stats()["symbolic_reused"] == 1 and {k: p.stats()[k] for k in topo} == before      # the planner did not run again
    fresh = fm.build(lib, x3, chain["plain"], fixed=(3,)); pf = _param(lib)
    fresh.cholesky(pf)
    assert _same_bits(g.states(), fresh.states()) and _same_bits(g.deltas(), fresh.deltas())
    _check_fixed_untouched(g, x3, (3,), "after fixing node 3")
    g.cholesky(p); fresh.cholesky(pf)                                       # (the fixed set's own captured graph)
    assert _same_bits(g.states(), fresh.states())
    # free it again: the bits of the graph that never had a fixed node (d_lambda's host cache was dropped with the set)
    x5 = g.states()
    _fix(g, (3,), False)
    g.cholesky(p)
    assert p.stats()["symbolic_reused"] == 1 and {k: p.stats()[k] for k in topo} == before
    never = fm.build(lib, x5, chain["plain"]); pn = _param(lib)
    never.cholesky(pn)
    assert _same_bits(g.states(), never.states()) and _same_bits(g.deltas(), never.deltas())
    assert not np.all(g.deltas()[3] == 0.0)
    for gg, pp in ((g, p), (fresh, pf), (never, pn)):
        pp.destroy(); gg.destroy()


def test_a_graph_that_never_had_a_fixed_node_keeps_its_captured_graph(lib, chain):
    runs = []
    for _ in range(2):
        g = fm.build(lib, chain["start"], chain["plain"]); p = _param(lib)
        for _ in range(5):
            g.cholesky(p)
        runs.append((g.states(), p.graph_captures()))
        p.destroy(); g.destroy()
    assert _same_bits(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1] == 1, runs                               # one capture (the second call's), replayed from then on


# ---- 4. resident loop equals API calls, bitwise -------------------------------------------------------------------------------------
def test_resident_loop_equals_api_calls(lib, chain):
    fixed = (0, 4)
    g = fm.build(lib, chain["start"], chain["plain"], fixed=fixed); p = _param(lib)
    for _ in range(5):
        g.cholesky(p)
    gr = fm.build(lib, chain["start"], chain["plain"], fixed=fixed); pr = _param(lib)
    chi, _ = gr.batch_resident(pr, 5)
    assert _same_bits(gr.states(), g.states()) and chi[-1] == g.chi2()
    _check_fixed_untouched(gr, chain["start"], fixed, "resident loop")
    x, plain = chain["start"], chain["plain"]
    for _ in range(5):
        A, B = fm.system(x, plain, lam=TIK)
        x = fm.step(x, fm.reduced_solve(A, B, fixed))
    _states_close(gr.states(), x, "five steps against the model")
    for gg, pp in ((g, p), (gr, pr)):
        pp.destroy(); gg.destroy()


# ---- 5. every kernel path ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(lib):
    states, fa, fb, z, W = datasets.random_pose_graph(700, 600, 21)
    N = len(states)
    fixed = np.sort(np.random.default_rng(11).permutation(N)[:120])
    fx = np.zeros(N, bool); fx[fixed] = True
    records = int(np.sum(fx[fa] | ((fb >= 0) & fx[np.where(fb >= 0, fb, 0)])))
    assert records > 256                                                    # k_fix_mask runs more than one workgroup
    P = PlanView(lib, N, fa, fb, xy=states[:, :2])
    own = lambda t: P.perm[P.front_first[t]:P.front_first[t] + P.front_nsb[t]]
    root = np.concatenate([own(t) for t in np.nonzero(P.front_parent < 0)[0]])
    leaf = np.concatenate([own(t) for t in np.nonzero(P.front_level == 0)[0]])
    assert fx[root].any() and fx[leaf].any() and not fx[root].all() and not fx[leaf].all()
    plain = (np.asarray(fa, np.int64), np.asarray(fb, np.int64), z, W)
    A, B = fm.system(states, plain, lam=TIK)
    d = fm.reduced_solve(A, B, fixed)
    return dict(states=states, arrays=(fa, fb, z, W), fixed=fixed, dx=d.reshape(-1, 3), x1=fm.step(states, d))


def _big_step(lib, big):
    g = lib.new_graph(); g.build_from_arrays(big["states"], *big["arrays"])
    _fix(g, big["fixed"])
    p = _param(lib)
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    out = (g.deltas(), g.states())
    p.destroy(); g.destroy()
    return out


@pytest.mark.parametrize("opts", KERNEL_PATHS + [dict(pool_guard=64), dict(pool_poison=1)], ids=_ids)
def test_every_kernel_path(lib, big, opts):
    assert dict(linearize_staged_min=0) in KERNEL_PATHS
    with lib.options(**opts):
        dx, st = _big_step(lib, big)
    _close(dx, big["dx"], f"{_ids(opts)}: dx against the reduced dense solve")
    _states_close(st, big["x1"], f"{_ids(opts)}: states")
    f = big["fixed"]
    assert np.all(dx[f] == 0.0) and _same_bits(st[f, :2], big["states"][f, :2])


# ---- 6. what writes the slot before the mask ---------------------------------------------------------------------------------------
def _slot_writer_case(lib, make, fixed):
    """make() -> a fresh graph with nobody fixed.  The bitwise A / B comparison of test 1 against that graph, then one step against the
    reduced solve of its A / B"""
    g0 = make(); p0 = _param(lib)
    A0, B0 = _stage(lib, g0, p0)
    x0 = g0.states()
    g = make(); _fix(g, fixed); p = _param(lib)
    A, B = _stage(lib, g, p)
    wantA, wantB = fm.mask(A0, B0, fixed)
    assert _same_bits(A, wantA) and _same_bits(B, wantB)
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    d = fm.reduced_solve(A0, B0, fixed)
    _close(g.deltas(), d.reshape(-1, 3), "dx against the reduced solve of the unmasked A / B")
    for i in fixed:
        assert np.all(g.deltas()[i] == 0.0) and _same_bits(g.states()[i, :2], x0[i, :2])
    for gg, pp in ((g, p), (g0, p0)):
        pp.destroy(); gg.destroy()


def test_robust_closure_on_a_fixed_node(lib, chain):
    def make():
        g = fm.build(lib, chain["start"], chain["plain"])
        assert (chain["plain"][0][7], chain["plain"][1][7]) == (0, 4)
        assert g.set_robust(7, abi.ROBUST_CAUCHY, 0.5) == 0 and g.set_robust(9, abi.ROBUST_HUBER, 0.1) == 0      # the closure (0, 4), the prior on 5
        return g
    _slot_writer_case(lib, make, (0,))
    _slot_writer_case(lib, make, (5,))


def test_max_mixture_closure_on_a_fixed_node(lib, chain):
    fa, fb, z, W = chain["plain"]
    keep = np.ones(len(fa), bool); keep[[7, 8]] = False

    def make():
        g = fm.build(lib, chain["start"], tuple(v[keep] for v in chain["plain"]))
        for k in (7, 8):
            g.add_factor_max(int(fa[k]), int(fb[k]), *maxmix_model.two_component(z[k], W[k]))
        return g
    _slot_writer_case(lib, make, (4,))


def test_polar_factor_on_a_fixed_node(lib, chain):
    x = chain["start"]
    polars = [(pm.RANGE_BEARING, 0, 6, pm.h(pm.RANGE_BEARING, pm.rel(x[0], x[6])[0]) + [0.03, -0.01], np.diag([400.0, 2500.0])),
              (pm.RANGE, 6, 2, pm.h(pm.RANGE, pm.rel(x[6], x[2])[0]) + [0.02], np.array([[300.0]]))]
    _slot_writer_case(lib, lambda: fm.build(lib, x, chain["plain"], polars=polars), (6,))
    _slot_writer_case(lib, lambda: fm.build(lib, x, chain["plain"], polars=polars), (0, 2))


def test_asymmetric_w_factor_on_a_fixed_node(lib):
    arr = asym_scenarios.batch_graph(n=24, extra=14, seed=11)
    W = arr[4].reshape(-1, 3, 3)
    assert np.any(W[:, 0, 1] != W[:, 1, 0])

    def make():
        g = lib.new_graph(); g.build_from_arrays(*arr)
        return g
    _slot_writer_case(lib, make, (0, 7, 8))


def _midpoint_blocks(x, nodes, z, W):
    """J [3][2, 3] and r [2] of tests/support/custom_factor.c's three-pose midpoint factor at x"""
    pa, pb, pc = (x[i] for i in nodes)
    c, s = np.cos(pa[2]), np.sin(pa[2])
    d = pb[:2] - 0.5 * (pa[:2] + pc[:2])
    h = np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])
    R = np.array([[c, s], [-s, c]])
    J = [np.column_stack([-0.5 * R, [h[1], -h[0]]]), np.column_stack([R, [0, 0]]), np.column_stack([-0.5 * R, [0, 0]])]
    return J, np.asarray(z) - h


def test_host_evaluated_three_node_factor_on_a_fixed_node(lib, chain, tmp_path):
    """A three-pose foreign factor is a clique of three packed entries: fixing one of its poses zeroes the slots of the two entries that
    hold it.  aprilsam_amd_debug_stage refuses host-evaluated factors (-4, as before), so A and B of this case are the numpy model's."""
    cl = custom_scenario.build_custom_lib(str(tmp_path))
    x0 = chain["start"]
    nodes, z, W = (1, 6, 3), np.array([0.4, -0.2]), np.array([[50.0, 5.0], [5.0, 40.0]])
    A, B = fm.system(x0, chain["plain"], lam=TIK)
    J, r = _midpoint_blocks(x0, nodes, z, W)
    for i, Ji in zip(nodes, J):
        B[3 * i:3 * i + 3] += Ji.T @ W @ r
        for j, Jj in zip(nodes, J):
            A[3 * i:3 * i + 3, 3 * j:3 * j + 3] += Ji.T @ W @ Jj
    for fixed in ((6,), (1, 3), (0,)):
        g = fm.build(lib, x0, chain["plain"])
        lib._add_factor(g.ptr, cl.custom_midpoint_create(*nodes, (C.c_double * 2)(*z), (C.c_double * 4)(*W.reshape(4))))
        _fix(g, fixed)
        p = _param(lib)
        lib.clear_error()
        g.cholesky(p)
        assert lib.last_error()[0] == 0 and p.stats()["not_spd"] == 0
        d = fm.reduced_solve(A, B, fixed)
        _close(g.deltas(), d.reshape(-1, 3), f"{fixed}: dx with the three-pose factor")
        _check_fixed_untouched(g, x0, fixed, fixed)
        p.destroy(); g.destroy()


# ---- 7. LM -------------------------------------------------------------------------------------------------------------------------
def test_lm_one_iteration(lib, chain):
    x0, plain, fixed, lam0 = chain["start"], chain["plain"], (0, 7), 1e-2
    g = fm.build(lib, x0, plain, fixed=fixed); p = _param(lib)
    r = g.optimize_lm(p, max_iters=1, lambda0=lam0)
    assert r["accepted"] == 1 and r["iterations"] == 1
    A, B = fm.system(x0, plain, lam=0.0)
    d = fm.reduced_solve(A, B, fixed, extra_diag=lam0)                       # LM's damping never reaches a fixed node
    _states_close(g.states(), fm.step(x0, d), "states after one LM iteration")
    _close(g.deltas(), d.reshape(-1, 3), "the accepted h")
    _close(r["F_final"], lm_model.cost(g.states(), plain), "F_final")
    _check_fixed_untouched(g, x0, fixed, "LM")
    p.destroy(); g.destroy()


def test_lm_to_convergence(lib):
    sc = gm.snake(4, 0, 3)
    x0, plain, fixed = sc["start"], sc["plain"], (0,)
    assert len(x0) == 16 and fm.unchanged_by_wrap(x0[0, 2])
    g = fm.build(lib, x0, plain, fixed=fixed); p = _param(lib)
    r = g.optimize_lm(p)
    assert r["status"] in (lm_model.CONVERGED_F, lm_model.CONVERGED_X), r
    x = g.states()
    _close(r["F_final"], lm_model.cost(x, plain), "F_final against numpy at the returned states")
    assert _same_bits(x[0], x0[0]) and np.all(g.deltas()[0] == 0.0)
    # every factor still counts: the prior on the fixed node 0 is in F and in chi2
    _close(r["chi2_final"], pm.chi2(x, plain, []), "chi2_final")
    g.cholesky(p)                                                          # one more plain step from there
    A, B = fm.system(x, plain, lam=TIK)
    d = fm.reduced_solve(A, B, fixed)
    _close(g.deltas(), d.reshape(-1, 3), "a plain step from the optimum")
    _states_close(g.states(), fm.step(x, d), "states after it")
    assert _same_bits(g.states()[0], x0[0])
    p.destroy(); g.destroy()


# ---- 8. GNC ------------------------------------------------------------------------------------------------------------------------
def test_gnc(lib):
    sc = gm.snake(*gm.CASES[0])
    x0, plain, fixed = sc["start"], sc["plain"], (0,)
    assert len(x0) == 16 and sc["is_false"].sum() == 3 and fm.unchanged_by_wrap(x0[0, 2])
    g = fm.build(lib, x0, plain, fixed=fixed); p = _param(lib)
    r = g.optimize_gnc(p, sc["cand"], loss=abi.GNC_TLS)
    assert r["status"] == 1, r
    x = g.states()
    assert _same_bits(x[0], x0[0]) and np.all(g.deltas()[0] == 0.0)
    F = gm.cost(x, plain, sc["cand"], gm.TLS, gm.C_DEFAULT, r["mu_final"])
    _close(r["F_final"] / F, 1.0, "F_final against numpy at the returned states")
    s = gm.robust_model.s_of(x, plain)[sc["cand"]]
    _close(r["weights"], gm.weight(gm.TLS, gm.C_DEFAULT, r["mu_final"], s), "weights against numpy at the returned states", 1e-12)
    p.destroy(); g.destroy()


# ---- 9. consumers of the retained factor -------------------------------------------------------------------------------------------
def test_consumers(lib, chain):
    x0, plain, fixed = chain["start"], chain["plain"], (0, 7)
    g = fm.build(lib, x0, plain, fixed=fixed); p = _param(lib)
    g.cholesky(p)
    assert np.array_equal(g.l_points(), x0)
    A, B = fm.system(x0, plain, lam=TIK)
    S = fm.conditional_covariance(A, fixed)
    blk = lambda i, j: S[3 * i:3 * i + 3, 3 * j:3 * j + 3]
    joint = lambda i, j: np.block([[blk(i, i), blk(i, j)], [blk(j, i), blk(j, j)]])
    N = 8

    def zero_rows(J, a, b, what):
        for k, (i, j) in enumerate(zip(a, b)):
            m = np.zeros(6, bool); m[:3] = i in fixed; m[3:] = j in fixed
            assert _same_bits(J[k][m, :], np.zeros_like(J[k][m, :])) and _same_bits(J[k][:, m], np.zeros_like(J[k][:, m])), (what, i, j)

    cov = g.marginals(p)
    _close(cov, np.array([blk(i, i) for i in range(N)]), "marginals: blocks of inv(A_ff), zeros at the fixed nodes")
    for i in fixed:
        assert _same_bits(cov[i], np.zeros((3, 3)))
    sub = g.marginals(p, [7, 3, 0])
    assert _same_bits(sub, cov[[7, 3, 0]])
    a = np.array([0, 1, 6, 3, 0, 7], np.int32); b = np.array([1, 2, 7, 4, 4, 2], np.int32)       # (pairs that share a factor: on the factor's pattern)
    J = g.marginals_joint(p, a, b)
    assert not np.isnan(J).any()
    _close(J, np.array([joint(i, j) for i, j in zip(a, b)]), "marginals_joint")
    zero_rows(J, a, b, "marginals_joint")
    a = np.array([1, 2, 0, 7, 5, 0], np.int32); b = np.array([5, 0, 7, 7, 5, 3], np.int32)
    J = g.marginals_joint_any(p, a, b)
    _close(J, np.array([joint(i, j) for i, j in zip(a, b)]), "marginals_joint_any")
    zero_rows(J, a, b, "marginals_joint_any")
    # gating: (free, free), (free, fixed), (fixed, free), (fixed, fixed): Sigma of the fixed poses is 0
    ga = np.array([1, 2, 0, 0], np.int32); gb = np.array([5, 0, 6, 7], np.int32)
    rng = np.random.default_rng(4)
    st = g.states()
    zc = np.array([gate_model.predict(st[i], st[j]) for i, j in zip(ga, gb)]) + rng.normal(0, 0.05, (4, 3))
    Wc = np.tile(np.diag([100.0, 100.0, 400.0]).reshape(9), (4, 1))
    d2, Sg = g.gate_xyt(p, ga, gb, zc, Wc)
    want_d2, want_S = gate_model.gate(st, ga, gb, zc, Wc, np.array([joint(i, j) for i, j in zip(ga, gb)]))
    _close(Sg, want_S, "gate_xyt S")
    _close(d2, want_d2, "gate_xyt d2")
    _close(Sg[3], np.linalg.inv(Wc[3].reshape(3, 3)), "gate_xyt between two fixed poses: S = W^-1", 1e-12)
    # solve: the system that was factorised, identity blocks included
    Bq = rng.normal(0, 1, (2, 3 * N))
    X = g.solve(p, Bq, mode="full")
    Am, _ = fm.mask(A, B, fixed)
    _close(X, np.linalg.solve(Am, Bq.T).T, "solve FULL against the dense solve of the masked A")
    idx = fm.dofs(fixed)
    _close(X[:, idx], Bq[:, idx], "solve FULL: x of a fixed node is its right-hand side", 1e-15)
    # a toggle after the factorisation drops the retained factor: the consumers answer as without one
    _fix(g, (7,), False)
    with pytest.raises(host.MarginalsError) as e:
        g.marginals(p)
    assert e.value.code == -1
    g.cholesky(p)
    assert not _same_bits(g.marginals(p)[7], np.zeros((3, 3)))
    p.destroy(); g.destroy()


# ---- 10. every refusal ---------------------------------------------------------------------------------------------------------------
def _refused(lib, what):
    code, msg = lib.last_error()
    assert code == -12 and "node 0" in msg and "fixed" in msg, (what, code, msg)
    lib.clear_error()


def test_refusals(lib, chain):
    x0, plain = chain["start"], chain["plain"]
    g = fm.build(lib, x0, plain, fixed=(0,)); p = _param(lib)
    g.cholesky(p)
    st, lp = g.states(), g.l_points()
    dll = lib.dll

    def untouched(what):
        assert _same_bits(g.states()[:len(st)], st) and _same_bits(g.l_points()[:len(lp)], lp), what

    # the consumers that are not open yet: nothing written
    for name, fn in (("marginals_cross", g.marginals_cross), ("relative_covariances", g.relative_covariances)):
        lib.clear_error()
        with pytest.raises(host.MarginalsError) as e:
            fn(p, 1, [2, 3])
        assert e.value.code == -12
        _refused(lib, name)
        untouched(name)
    out = np.full((2, 3, 3), -7.0)
    idx = np.array([2, 3], np.int32)
    assert dll.aprilsam_amd_marginals_cross(g.ptr, p.ptr, 1, 2, host._np_i(idx), host._np_d(out)) == -12 and np.all(out == -7.0)
    lib.clear_error()
    # chordal initialisation
    co = abi.ChordalOpts(); dll.aprilsam_amd_chordal_opts_init(C.byref(co))
    crep = abi.ChordalReport(); crep.status = -77
    rot = np.full(2 * g.n_nodes, -7.0)
    assert dll.aprilsam_amd_initialize_chordal(g.ptr, p.ptr, C.byref(co), C.byref(crep), host._np_d(rot)) == -12
    assert np.all(rot == -7.0) and crep.status == -77
    _refused(lib, "initialize_chordal")
    untouched("initialize_chordal")
    # sharded runs
    dll.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    ps = lib.new_param()
    assert dll.aprilsam_amd_shard_begin(C.cast(g.ptr, C.c_void_p), C.cast(ps.ptr, C.c_void_p), 0, 1) == -12
    _refused(lib, "shard_begin")
    untouched("shard_begin")
    ps.destroy()
    # the incremental entry points (void: the refusal is aprilsam_amd_last_error's)
    g.cholesky_inc_solver(p)
    _refused(lib, "cholesky_inc_solver")
    untouched("cholesky_inc_solver")
    g.add_node_xyt([1.0, 1.0, 0.25])
    g.add_factor_xyt(7, 8, [1.0, 0.0, 0.7], np.diag([400.0, 400.0, 2500.0]))
    n8 = g.states()[8].copy()
    g.cholesky_inc(p)
    _refused(lib, "cholesky_inc")
    untouched("cholesky_inc")
    assert _same_bits(g.states()[8], n8)
    # with node 0 freed the graph itself is fine, but the factorisation at hand was made with node 0 fixed: a batch call comes first
    _fix(g, (0,), False)
    g.cholesky_inc(p)
    code, msg = lib.last_error()
    assert code == -12 and "node 0" in msg and "april_graph_cholesky" in msg, (code, msg)
    untouched("cholesky_inc on a factorisation made with a fixed node")
    lib.clear_error()
    # nothing above cost the param its use: batch, then incremental steps as ever
    g.cholesky(p)
    assert lib.last_error()[0] == 0 and p.stats()["not_spd"] == 0
    g.add_node_xyt([2.0, 1.0, 0.25])
    g.add_factor_xyt(8, 9, [1.0, 0.0, 0.0], np.diag([400.0, 400.0, 2500.0]))
    g.cholesky_inc(p)
    assert lib.last_error()[0] == 0
    p.destroy(); g.destroy()
