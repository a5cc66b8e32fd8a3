"""aprilsam_amd_initialize_chordal on the GPU: both stages against their exact linear systems (matrix-free, no
factorisation involved), the states against the numpy model (tests/support/chordal_model.py), exact recovery, what the start buys LM on
M3500, every kernel path, the smallest shapes, loss / mixture semantics, the contract the call leaves behind, and every refusal."""
import functools

import numpy as np
import pytest

from aprilsam_amd import abi, datasets
from aprilsam_amd.host import ChordalError, MarginalsError
from tests.support import chordal_model as CM
from tests.support import lm_model as M
from tests.support.marginal_cases import tutorial_arrays

pytestmark = pytest.mark.gpu

RES_RTOL = 1e-10        # tests/test_gpu_normal_eq.py: the project's tolerance for a solve
CASE_NAMES = ["m3500", "random0", "random1", "random2", "random3", "lattice24"]


@functools.lru_cache(maxsize=None)
def _arrays(name):
    if name == "m3500":
        st, fa, fb, z, W = datasets.m3500_batch()
    elif name.startswith("random"):
        st, fa, fb, z, W = datasets.random_pose_graph(300, 200, int(name[6:]))
    elif name.startswith("exact"):
        st, fa, fb, z, W = datasets.random_pose_graph(300, 200, int(name[5:]))
        z = CM.exact_measurements(st, fa, fb)
    else:
        from aprilsam_amd import host
        st, fa, fb, z, W = host.SolverLib().lattice_arrays(int(name[7:]))
    for v in (st, fa, fb, z, W):
        v.setflags(write=False)
    return st, (fa, fb, z, W)


@functools.lru_cache(maxsize=None)
def _model(name):
    """the model's result and its own spread s_case over spsolve's orderings (never taken from the library)"""
    st, plain = _arrays(name)
    zero = np.zeros_like(st)
    return CM.initialize(plain, zero), CM.spread(plain, zero)


def _graph(lib, states, fa, fb, z, W):
    g = lib.new_graph(); g.build_from_arrays(states, fa, fb, z, W)
    return g


def _run(lib, name, x_in=None, **kw):
    st, plain = _arrays(name)
    g = _graph(lib, np.zeros_like(st) if x_in is None else x_in, *plain); p = lib.new_param()
    r = g.initialize_chordal(p, **kw)
    x = g.states()
    assert x.tobytes() == g.l_points().tobytes()
    p.destroy(); g.destroy()
    return r, x


def _check_residuals(name, r, x):
    """r: a raw=True run.  Both stages' A u - B relative to the largest sum of |terms| of the stage's right-hand side; padding exactly 0"""
    st, plain = _arrays(name)
    raw = r["raw"]
    out = CM.residuals(plain, raw[0][:, :2], x)
    print(name, "rel1 %.3e rel2 %.3e  (|res| %.3e / %.3e, scales %.3e / %.3e)" % (out["rel1"], out["rel2"], out["res1"], out["res2"], out["scale1"], out["scale2"]))
    assert np.all(raw[:, :, 2] == 0), name
    assert x[:, :2].tobytes() == np.ascontiguousarray(raw[1][:, :2]).tobytes()
    assert np.abs(x[:, 2] - np.arctan2(raw[0][:, 1], raw[0][:, 0])).max() <= 2e-15        # (atan2 of the device against numpy's: a few ulps of pi)
    assert out["rel1"] <= RES_RTOL and out["rel2"] <= RES_RTOL, (name, out)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_both_stages_solve_their_linear_systems(lib, name):
    r, x = _run(lib, name, raw=True)
    assert r["status"] == 0 and r["not_spd_stage"] == 0 and r["n_degenerate"] == 0
    _check_residuals(name, r, x)
    # rot_out: the public counterpart of the raw solution's first two columns
    r2, x2 = _run(lib, name, rot=True)
    assert r2["rot"].tobytes() == np.ascontiguousarray(r["raw"][0][:, :2]).tobytes() and x2.tobytes() == x.tobytes()
    assert abs(r2["min_norm"] - np.sqrt((r2["rot"] ** 2).sum(axis=1).min())) <= 1e-15


@pytest.mark.parametrize("name", CASE_NAMES)
def test_states_match_the_model(lib, name):
    st, plain = _arrays(name)
    ref, s_case = _model(name)
    r, x = _run(lib, name)
    tol = max(1e-9, 10 * s_case)
    d = CM.state_diff(x, ref["x"])
    print(name, "max state difference %.3e, s_case %.3e, tolerance %.3e" % (d, s_case, tol))
    assert d <= tol, (name, d, tol)
    assert r["n_degenerate"] == ref["n_degenerate"] and abs(r["min_norm"] - ref["min_norm"]) <= 1e-9
    assert abs(r["F_initial"] - M.cost(np.zeros_like(st), plain)) <= 1e-12 * r["F_initial"]
    assert abs(r["F_final"] - M.cost(x, plain)) <= 1e-9 * r["F_final"]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_exact_measurements_are_recovered(lib, seed):
    name = f"exact{seed}"
    st, plain = _arrays(name)
    r0, x0 = _run(lib, name)
    garbage = np.random.default_rng(seed).uniform(-50.0, 50.0, st.shape)
    r1, x1 = _run(lib, name, x_in=garbage)
    d = CM.state_diff(x0, st)
    print(name, "max |state - truth| %.3e" % d)
    assert d <= 1e-9
    assert x0.tobytes() == x1.tobytes()                      # the result reads no incoming state
    assert r0["F_final"] == r1["F_final"] and r0["F_initial"] != r1["F_initial"]


def test_purpose_lm_reaches_the_optimum_from_zero_states(lib):
    st, plain = _arrays("m3500")
    g = _graph(lib, np.zeros_like(st), *plain); p = lib.new_param()
    g.initialize_chordal(p)
    r = g.optimize_lm(p)
    print("M3500 from zeros: chordal + LM", r["status"], r["iterations"], r["F_final"])
    assert r["status"] == abi.LM_CONVERGED_F and abs(r["F_final"] - 137.913) <= 1e-6 * 137.913
    g2 = _graph(lib, np.zeros_like(st), *plain); p2 = lib.new_param()
    r2 = g2.optimize_lm(p2)
    print("M3500 from zeros: LM alone", r2["status"], r2["iterations"], r2["F_final"])
    assert not (r2["status"] == abi.LM_CONVERGED_F and abs(r2["F_final"] - 137.913) <= 1e-6 * 137.913)
    for o in (p, g, p2, g2):
        o.destroy()


# The stage solves under the batch step's kernel paths: without a captured graph, fronts on the multi-workgroup and panel paths, both
# back-substitution forms, per-level launches, unplaced fronts, the front pool poisoned / guard-banded, the staged linearisation's threshold
PATHS = [dict(use_graph=0), dict(small_lds_kb=0), dict(small_lds_kb=48), dict(wave_backsolve=0), dict(blk_backsolve=0, small_lds_kb=0),
         dict(persist=0), dict(xcd_place=0), dict(pool_poison=1), dict(pool_guard=64), dict(linearize_staged_min=0)]
# the same kernels in the same order as the default run: the states bitwise
BITWISE = [dict(use_graph=0), dict(xcd_place=0), dict(pool_poison=1), dict(pool_guard=64)]


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items())


@functools.lru_cache(maxsize=None)
def _default_bits(name):
    from aprilsam_amd import host
    return _run(host.SolverLib(), name)[1].tobytes()


@pytest.mark.parametrize("opts", PATHS, ids=_ids)
@pytest.mark.parametrize("name", ["random0", "m3500"])
def test_residuals_on_every_kernel_path(lib, name, opts):
    with lib.options(**opts):
        r, x = _run(lib, name, raw=True)
    _check_residuals(name, r, x)
    if opts in BITWISE:
        assert x.tobytes() == _default_bits(name), (name, opts)


@pytest.mark.parametrize("name", ["random0", "m3500"])
def test_two_runs_give_identical_bits(lib, name):
    assert _run(lib, name)[1].tobytes() == _default_bits(name)


W_PRIOR = np.diag([100.0, 100.0, 400.0]).reshape(9)
W_ODO = np.diag([25.0, 25.0, 900.0]).reshape(9)


def _small(lib, arrays, **kw):
    st, fa, fb, z, W = arrays
    plain = (np.array(fa, np.int32), np.array(fb, np.int32), np.array(z, float).reshape(-1, 3), np.array(W, float).reshape(-1, 9))
    x_in = np.array(st, float)
    g = _graph(lib, x_in, *plain); p = lib.new_param()
    r = g.initialize_chordal(p, raw=True, **kw)
    x = g.states()
    p.destroy(); g.destroy()
    return r, x, plain


def test_one_pose_one_prior(lib):
    r, x, plain = _small(lib, ([[5.0, 5.0, 5.0]], [0], [-1], [[1.0, -2.0, 0.7]], [W_PRIOR]))
    assert np.abs(x - [[1.0, -2.0, 0.7]]).max() <= 1e-14 and np.all(r["raw"][:, :, 2] == 0)
    assert abs(r["min_norm"] - 1.0) <= 1e-15 and r["F_final"] <= 1e-25


def test_two_poses_prior_and_one_factor(lib):
    r, x, plain = _small(lib, (np.zeros((2, 3)), [0, 0], [-1, 1], [[1.0, 2.0, 0.5], [2.0, 0.0, -0.25]], [W_PRIOR, W_ODO]))
    c, s = np.cos(0.5), np.sin(0.5)
    want = np.array([[1.0, 2.0, 0.5], [1.0 + 2.0 * c, 2.0 + 2.0 * s, 0.25]])
    assert CM.state_diff(x, want) <= 1e-14, x
    out = CM.residuals(plain, r["raw"][0][:, :2], x)
    assert out["rel1"] <= RES_RTOL and out["rel2"] <= RES_RTOL and np.all(r["raw"][:, :, 2] == 0)


def test_tutorial_graph(lib):
    arrays = tutorial_arrays()
    r, x, plain = _small(lib, arrays)
    out = CM.residuals(plain, r["raw"][0][:, :2], x)
    assert out["rel1"] <= RES_RTOL and out["rel2"] <= RES_RTOL and np.all(r["raw"][:, :, 2] == 0)
    ref = CM.initialize(plain, np.zeros((6, 3)))
    assert CM.state_diff(x, ref["x"]) <= max(1e-9, 10 * CM.spread(plain, np.zeros((6, 3))))


def test_heading_free_prior_alone_is_refused_in_stage_1(lib):
    st, fa, fb, z, W = tutorial_arrays()
    W = np.array(W, float); W[0, 8] = 0.0
    g = _graph(lib, st, fa, fb, z, W); p = lib.new_param()
    before = (g.states().copy(), g.l_points().copy(), g.deltas().copy())
    with pytest.raises(ChordalError) as e:
        g.initialize_chordal(p)
    assert e.value.code == -2 and e.value.report["not_spd_stage"] == 1 and e.value.report["status"] == -2
    assert lib.last_error()[0] == -2
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (g.states(), g.l_points(), g.deltas())))
    g.cholesky(p)                                            # the graph and the param stay usable
    assert p.stats()["error_code"] == 0
    p.destroy(); g.destroy()


def test_no_position_prior_is_refused_in_stage_2(lib):
    st, fa, fb, z, W = tutorial_arrays()
    W = np.array(W, float); W[0, :8] = 0.0                   # a heading-only prior: stage 1 is anchored, stage 2 is not
    g = _graph(lib, st, fa, fb, z, W); p = lib.new_param()
    before = g.states().copy()
    with pytest.raises(ChordalError) as e:
        g.initialize_chordal(p)
    assert e.value.code == -2 and e.value.report["not_spd_stage"] == 2
    assert g.states().tobytes() == before.tobytes() and g.l_points().tobytes() == before.tobytes()
    p.destroy(); g.destroy()


def test_xy_only_prior_plus_heading_only_prior(lib):
    st, fa, fb, z, W = tutorial_arrays()
    W = np.array(W, float); z = np.array(z, float)
    W[0, 8] = 0.0; z[0] = [0.5, -0.5, 3.0]                   # xy-only prior on pose 0 (its heading says nothing)
    fa = np.append(fa, 3).astype(np.int32); fb = np.append(fb, -1).astype(np.int32)
    z = np.vstack([z, [9.0, 9.0, 0.3]]); W = np.vstack([W, np.diag([0.0, 0.0, 50.0]).reshape(9)])      # heading-only prior on pose 3
    r, x, plain = _small(lib, (st, fa, fb, z, W))
    out = CM.residuals(plain, r["raw"][0][:, :2], x)
    assert out["rel1"] <= RES_RTOL and out["rel2"] <= RES_RTOL and np.all(r["raw"][:, :, 2] == 0)
    ref = CM.initialize(plain, np.zeros((6, 3)))
    assert CM.state_diff(x, ref["x"]) <= max(1e-9, 10 * CM.spread(plain, np.zeros((6, 3))))
    assert abs(x[3, 2] - 0.3) <= 1e-12 and np.abs(x[0, :2] - [0.5, -0.5]).max() <= 1e-12


def test_stages_1_leaves_positions_untouched(lib):
    st, plain = _arrays("random0")
    x_in = np.random.default_rng(3).uniform(-5.0, 5.0, st.shape)
    r1, x1 = _run(lib, "random0", x_in=x_in, stages=1)
    assert x1[:, :2].tobytes() == np.ascontiguousarray(x_in[:, :2]).tobytes()
    assert x1[:, 2].tobytes() == _run(lib, "random0")[1][:, 2].tobytes()


def _loop_graph():
    """random0 with one long loop closure appended"""
    st, (fa, fb, z, W) = _arrays("random0")
    zl = CM.exact_measurements(st, [10], [250])[0] + [0.05, -0.03, 0.02]
    return st, (fa, fb, z, W), (10, 250, zl, np.array(W[1]))


def test_a_robust_loss_is_ignored(lib):
    st, plain, (a, b, zl, Wl) = _loop_graph()
    bits = []
    for kind in (abi.ROBUST_NONE, abi.ROBUST_CAUCHY):
        g = _graph(lib, np.zeros_like(st), *plain); p = lib.new_param()
        g.add_factor_xyt(a, b, zl, Wl.reshape(3, 3))
        if kind:
            assert g.set_robust(g.n_factors - 1, kind, 1.0) == 0
        g.cholesky(p)                                        # (the robust factor's slot now holds a weighted W; the states move)
        g.set_all_states(np.zeros_like(st), relinearize=True)
        g.initialize_chordal(p)
        bits.append(g.states().tobytes())
        p.destroy(); g.destroy()
    assert bits[0] == bits[1]


def test_a_max_factor_enters_as_its_heaviest_component(lib):
    st, plain, (a, b, zl, Wl) = _loop_graph()
    g = _graph(lib, np.zeros_like(st), *plain); p = lib.new_param()
    g.add_factor_xyt(a, b, zl, Wl.reshape(3, 3))
    g.initialize_chordal(p)
    want = g.states().tobytes()
    p.destroy(); g.destroy()
    # [nominal, null hypothesis with the lower log weight], and the same two the other way round
    for order in ((0, 1), (1, 0)):
        zs = [zl, zl + [3.0, 3.0, 1.0]]; Ws = [Wl, 1e-6 * Wl]; lw = [np.log(0.9), np.log(0.1)]
        g = _graph(lib, np.zeros_like(st), *plain); p = lib.new_param()
        g.add_factor_max(a, b, [zs[k] for k in order], [Ws[k] for k in order], [lw[k] for k in order])
        g.initialize_chordal(p)
        assert g.states().tobytes() == want, order
        p.destroy(); g.destroy()


def test_contract_and_non_interference(lib):
    st, plain = _arrays("m3500")
    x0 = M.perturbed(st, 0.3)
    g = _graph(lib, x0, *plain); p = lib.new_param()
    g.cholesky(p)
    dx_before = g.deltas().copy()
    assert g.marginals(p) is not None
    g.initialize_chordal(p)
    xs = g.states()
    assert xs.tobytes() == g.l_points().tobytes() and g.deltas().tobytes() == dx_before.tobytes() and p.c.tikhanov == 1e-4
    with pytest.raises(MarginalsError) as e:
        g.marginals(p)
    assert e.value.code == -1
    # the next plain step: the bits of a fresh param that never ran the initialisation, given the same states (and, as the plan takes a
    # hint from the coordinates it is made at, made at the same start: tests/test_gpu_lm.py's contract test)
    gr = _graph(lib, x0, *plain); pr = lib.new_param(); gr.cholesky(pr)
    gr.set_all_states(xs, relinearize=True)
    g.cholesky(p); gr.cholesky(pr)
    assert g.states().tobytes() == gr.states().tobytes() and g.deltas().tobytes() == gr.deltas().tobytes()
    assert g.marginals(p).tobytes() == gr.marginals(pr).tobytes()
    for o in (p, g, pr, gr):
        o.destroy()


def test_every_refusal_leaves_the_graph_and_param_usable(lib, tmp_path):
    import ctypes as C
    from tests.support import custom_scenario
    from tests.support.asym_scenarios import batch_graph
    arr = datasets.random_pose_graph(200, 100, 5)
    x0 = M.perturbed(arr[0], 0.3, 5)

    def check(g, p, code, **kw):
        s, l, d = g.states().copy(), g.l_points().copy(), g.deltas().copy()
        with pytest.raises(ChordalError) as e:
            g.initialize_chordal(p, **kw)
        assert e.value.code == code and lib.last_error()[0] == code
        assert s.tobytes() == g.states().tobytes() and l.tobytes() == g.l_points().tobytes() and d.tobytes() == g.deltas().tobytes()

    g = _graph(lib, x0, *arr[1:]); p = lib.new_param()
    for bad in (dict(stages=0), dict(stages=2)):
        check(g, p, -13, **bad)
    check(g, None, -13)
    ge = lib.new_graph()
    check(ge, p, -1)
    assert g.initialize_chordal(p)["status"] == 0
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
    assert gs.initialize_chordal(ps)["status"] == 0
    for o in (p, g, ge, ph, gh, pa, ga, ps, gs):
        o.destroy()
