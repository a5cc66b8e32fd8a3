"""Joint covariances of any pose pair (aprilsam_amd_marginals_joint_any) and gating of candidate xyt measurements
(aprilsam_amd_gate_xyt) on the GPU: path solves of the retained factor (aprilsam_amd/csrc/pathsolve.hip.h).  Checked against numpy's
inverse of the system the step factorised, the selected inversion on the pattern of L, splu solves at 10^5 poses, the numpy gating model
(tests/support/gate_model.py), through the M3500 incremental demo; bitwise repeatability, non-interference and the error returns."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets, harness
from tests.support.gate_model import CHI2_3_999, gate, gate_inputs as _gate_inputs, held_out_closures
from tests.support.marginal_cases import case_arrays, factor_pairs
from tests.support.selinv_model import dense_system, sparse_system, system_blocks
from tests.support.sigma_compare import (SIG_RTOL, Recorder, compare_dense_any as _compare_dense, demo_checkpoints, dense as _dense,
                                         random_pairs as _pairs, ref_joint as _ref_joint)
from tests.test_pathsolve_model import FALSE_REJECTED, GATE_ITERS, TRUE_ACCEPTED, m3500_gate_scenario

pytestmark = pytest.mark.gpu
# SIG_RTOL = 1e-9 against the dense inverse, of the two poses' block rows' largest entry (tests/support/sigma_compare.py)
SPLU_RTOL = 1e-8         # against splu solves (10^5-pose lattice; tests/test_gpu_marginals.py)
GATE_RTOL = 1e-9         # d2 and S against the numpy model


def _solved(lib, arr, steps=1):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    for _ in range(steps):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
    return g, p


def _heldout_m3500():
    arr = datasets.m3500_batch()
    cl, ho = held_out_closures(arr, 100)
    return arr, cl, ho


@pytest.mark.parametrize("name", ["tutorial", "random0", "random1", "random2", "random3", "lattice60", "m3500"])
def test_joint_any_matches_the_dense_inverse(lib, name):
    if name == "m3500":
        arr, cl, ho = _heldout_m3500()
        extra = (arr[1][cl], arr[2][cl])
        arr = ho
    else:
        arr = case_arrays(lib, name); extra = ([], [])
    g, p = _solved(lib, arr)
    N = len(arr[0])
    a, b = _pairs(N, 1)
    fa, fb = factor_pairs(arr[1], arr[2])
    a = np.r_[a, extra[0], fa].astype(np.int32); b = np.r_[b, extra[1], fb].astype(np.int32)
    J = _compare_dense(g, p, a, b)
    on = g.marginals_joint(p, a, b)                            # on the pattern: the selected inversion's blocks
    m = ~np.isnan(on).any(axis=(1, 2))
    assert m.sum() >= len(fa)
    Sig, scale = _dense(g, p)
    err = np.abs(J[m] - on[m]).reshape(-1, 36).max(axis=1) / np.maximum(scale[a[m]], scale[b[m]])
    assert err.max() < SIG_RTOL
    p.destroy(); g.destroy()


def test_lattice_100k_against_sparse_solves(lib):
    import scipy.sparse.linalg as sla
    arr = lib.lattice_arrays(316)
    g, p = _solved(lib, arr)
    states, fa, fb, z, W = arr
    N = len(states)
    a, b = _pairs(N, 2, 32)
    a, b = a[:64], b[:64]
    J = g.marginals_joint_any(p, a, b)
    Aii, Aab = system_blocks(g.l_points(), fa, fb, z, W, p.c.tikhanov)
    lu = sla.splu(sparse_system(Aii, Aab, fa, fb).tocsc())
    for i in range(len(a)):
        E = np.zeros((3 * N, 6)); E[3 * a[i]:3 * a[i] + 3, :3] = np.eye(3); E[3 * b[i]:3 * b[i] + 3, 3:] = np.eye(3)
        X = lu.solve(E)
        ix = np.r_[3 * a[i]:3 * a[i] + 3, 3 * b[i]:3 * b[i] + 3]
        assert np.abs(J[i] - X[ix]).max() < SPLU_RTOL * np.abs(X).max(), i
    p.destroy(); g.destroy()


def test_lattice_1m_agrees_with_the_selected_inversion_and_runs_none(lib):
    arr = lib.lattice_arrays(1000)
    g, p = _solved(lib, arr)
    N = len(arr[0])
    fa, fb = factor_pairs(arr[1], arr[2])
    rng = np.random.default_rng(4)
    k = rng.choice(len(fa), 64, replace=False)
    a, b = fa[k].astype(np.int32), fb[k].astype(np.int32)
    r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    J = g.marginals_joint_any(p, a, b)
    Jr = g.marginals_joint_any(p, b, a)
    z = np.zeros((len(a), 3)); W = np.tile(np.eye(3).ravel() * 100, (len(a), 1))
    g.gate_xyt(p, a, b, z, W)
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0           # no selected inversion for joint_any or gating
    assert lib.dll.aprilsam_amd_debug_path_solve_bytes(p.ptr) < (2 << 30)
    sw = np.r_[3:6, 0:3]
    assert np.array_equal(Jr, J[:, sw][:, :, sw])
    on = g.marginals_joint(p, a, b)
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0 + 1
    d = g.marginals(p, np.r_[a, b])
    scale = np.abs(d).reshape(2, len(a), 9).max(axis=(0, 2))
    err = np.abs(J - on).reshape(len(a), 36).max(axis=1) / scale
    assert err.max() < SIG_RTOL, err.max()
    p.destroy(); g.destroy()


def test_incremental_demo_checkpoints_and_non_interference(lib):
    """First 600 steps of the M3500 incremental demo, the checkpoints of tests/test_gpu_marginals.py: joint_any of random pairs, the
    newest pose against old ones, and a == b, against inv(A(l_point)) with lambda on the poses of the last batch step; the chi^2 trace
    and states bitwise those of the run without the calls."""
    arr = datasets.m3500_arrays()
    plain = harness.run_demo(lib, arr, max_poses=600, record_states_every=50)
    rec = Recorder(lib)

    def check(g, p, k, lam_nodes):
        N = g.n_nodes
        a, b = _pairs(N, k, 20)
        a = np.r_[a, np.full(min(N, 20), N - 1)].astype(np.int32); b = np.r_[b, np.arange(min(N, 20))].astype(np.int32)
        _compare_dense(g, p, a, b, lam_nodes)
    on_step, seen = demo_checkpoints(rec, arr, check)
    res = harness.run_demo(rec, arr, max_poses=600, record_states_every=50, on_step=on_step)
    assert seen["batch"] >= 5 and seen["updated"] >= 1 and seen["fast"] >= 12, seen
    assert res["chi2"].tobytes() == plain["chi2"].tobytes()
    assert res["final_states"].tobytes() == plain["final_states"].tobytes()
    for k in plain["snaps"]:
        assert res["snaps"][k].tobytes() == plain["snaps"][k].tobytes()


def test_after_batch_resident(lib):
    arr = case_arrays(lib, "random1")
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.batch_resident(p, 3)
    a, b = _pairs(len(arr[0]), 9)
    _compare_dense(g, p, a, b)
    p.destroy(); g.destroy()


def test_gate_matches_the_model(lib):
    arr = case_arrays(lib, "random2")
    g, p = _solved(lib, arr, 2)
    a, b, z, W = _gate_inputs(arr, 300, 5)
    d2, S = g.gate_xyt(p, a, b, z, W)
    J = g.marginals_joint_any(p, a, b)
    md2, mS = gate(g.states(), a, b, z, W, J)
    assert np.abs(d2 - md2).max() < GATE_RTOL * np.abs(md2).max() and (np.abs(d2 - md2) <= GATE_RTOL * np.abs(md2) + 1e-300).all()
    assert np.abs(S - mS).max() < GATE_RTOL * np.abs(mS).max()
    Sig, _ = _dense(g, p)                                      # (and the model with the dense inverse's blocks)
    md2b, _ = gate(g.states(), a, b, z, W, _ref_joint(Sig, a, b))
    assert (np.abs(d2 - md2b) <= 1e-7 * np.abs(md2b)).all()
    p.destroy(); g.destroy()


def test_gating_end_to_end_on_m3500(lib):
    """M3500 solved without its last 100 loop closures; the held-out closures and 100 false candidates (a true closure's z, W on a wrong
    pair of poses at least 50 apart) gated at chi2_3(0.999): the GPU decides as the CPU model does, at the rates recorded on the CPU"""
    ho, a, b, z, W = m3500_gate_scenario(None)
    g, p = _solved(lib, ho, GATE_ITERS)
    d2, S = g.gate_xyt(p, a, b, z, W)
    md2, mS, _ = m3500_gate_scenario(g.states(), g.l_points())
    acc = d2 < CHI2_3_999
    assert np.array_equal(acc, md2 < CHI2_3_999)
    assert int(acc[:100].sum()) == TRUE_ACCEPTED and int((~acc[100:]).sum()) == FALSE_REJECTED
    assert (np.abs(d2 - md2) <= 1e-7 * md2).all()
    p.destroy(); g.destroy()


def test_repeatability_and_non_interference(lib):
    arr = case_arrays(lib, "lattice60")
    g, p = _solved(lib, arr)
    N = len(arr[0])
    a, b = _pairs(N, 3)
    r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    m1 = g.marginals(p)
    j1 = g.marginals_joint_any(p, a, b); j2 = g.marginals_joint_any(p, a, b)
    assert j1.tobytes() == j2.tobytes()
    ga, gb, z, W = _gate_inputs(arr, 50, 1)
    d1, S1 = g.gate_xyt(p, ga, gb, z, W); d2, S2 = g.gate_xyt(p, ga, gb, z, W)
    assert d1.tobytes() == d2.tobytes() and S1.tobytes() == S2.tobytes()
    m2 = g.marginals(p)
    assert m1.tobytes() == m2.tobytes() and lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0 + 1
    g2, p2 = _solved(lib, arr)                                  # a fresh param: the same bits
    assert g2.marginals_joint_any(p2, a, b).tobytes() == j1.tobytes()
    for x in (p, g, p2, g2):
        x.destroy()


def test_batch_steps_are_bitwise_unaffected_by_gating(lib):
    arr = datasets.random_pose_graph(400, 350, 2)
    ga, gb, z, W = _gate_inputs(arr, 40, 2)
    runs = []
    for with_g in (False, True):
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        snaps = []
        for _ in range(10):
            g.cholesky(p)
            if with_g:
                g.gate_xyt(p, ga, gb, z, W); g.marginals_joint_any(p, ga, gb)
            snaps.append(np.concatenate([g.states(), g.deltas(), g.l_points()]).tobytes())
        runs.append(snaps)
        p.destroy(); g.destroy()
    assert runs[0] == runs[1]


def test_params_on_two_slots(lib):
    arr = case_arrays(lib, "lattice24")
    a, b = _pairs(len(arr[0]), 6)
    out = []
    for slots in ((0, 0), (0, 1)):
        gs, ps = [], []
        for s in slots:
            g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
            assert lib.dll.aprilsam_amd_param_set_device(p.ptr, s) == 0
            g.cholesky(p); gs.append(g); ps.append(p)
        j = [g.marginals_joint_any(p, a, b) for g, p in zip(gs, ps)]
        for g, p in zip(gs, ps):
            g.cholesky(p)
        out.append([j[0].tobytes(), j[1].tobytes()] + [g.states().tobytes() for g in gs])
        for x in gs + ps:
            x.destroy()
    assert out[0][0] == out[0][1] == out[1][0] == out[1][1]
    assert out[0][2:] == out[1][2:]


def test_error_returns_leave_everything_untouched(lib):
    from aprilsam_amd.host import MarginalsError
    arr = case_arrays(lib, "lattice24")
    N = len(arr[0])
    ref_g, ref_p = _solved(lib, arr, 2)
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    ga, gb, z, W = _gate_inputs(arr, 4, 3)

    def code(f, *args):
        with pytest.raises(MarginalsError) as e:
            f(*args)
        return e.value.code
    assert code(g.marginals_joint_any, p, [0], [1]) == -1 and code(g.gate_xyt, p, ga, gb, z, W) == -1     # a fresh param
    g.cholesky(p)
    r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    assert code(g.marginals_joint_any, p, [0], [N]) == -13 and code(g.marginals_joint_any, p, [-1], [0]) == -13
    assert code(g.gate_xyt, p, [0], [N], z[:1], W[:1]) == -13
    assert code(g.gate_xyt, p, [3], [3], z[:1], W[:1]) == -13                            # a == b
    bad = z.copy(); bad[2, 1] = np.nan
    assert code(g.gate_xyt, p, ga, gb, bad, W) == -13
    badW = W.copy(); badW[1, 4] = np.inf
    assert code(g.gate_xyt, p, ga, gb, z, badW) == -13
    asym = W.copy(); asym[0, 1] += 0.5
    assert code(g.gate_xyt, p, ga, gb, z, asym) == -12
    indef = W.copy(); indef[3] = np.diag([1.0, -1.0, 1.0]).ravel()
    assert code(g.gate_xyt, p, ga, gb, z, indef) == -12
    out = np.zeros((1, 6, 6))
    assert lib.dll.aprilsam_amd_marginals_joint_any(g.ptr, p.ptr, 1, None, None, out.ctypes.data_as(C.POINTER(C.c_double))) == -13
    d = lib.dll
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    d.aprilsam_amd_shard_end.argtypes = [C.c_void_p]
    g3, p3 = _solved(lib, arr)
    gp, pp = C.cast(g3.ptr, C.c_void_p), C.cast(p3.ptr, C.c_void_p)
    assert d.aprilsam_amd_shard_begin(gp, pp, 0, 1) == 0
    assert code(g3.marginals_joint_any, p3, [0], [1]) == -12 and code(g3.gate_xyt, p3, ga, gb, z, W) == -12
    d.aprilsam_amd_shard_end(pp)
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0
    one_g, one_p = _solved(lib, arr)                                                      # the next marginals call: as if none failed
    assert g.marginals(p).tobytes() == one_g.marginals(one_p).tobytes()
    g.cholesky(p)                                                                         # the next solver call: the same bits
    assert g.states().tobytes() == ref_g.states().tobytes()
    assert g.marginals(p).tobytes() == ref_g.marginals(ref_p).tobytes()
    assert g.marginals_joint_any(p, ga, gb).tobytes() == ref_g.marginals_joint_any(ref_p, ga, gb).tobytes()
    for x in (p, g, ref_p, ref_g, p3, g3, one_p, one_g):
        x.destroy()


def test_asymmetric_information_is_refused(lib):
    from aprilsam_amd.host import MarginalsError
    from tests.support.asym_scenarios import batch_graph
    arr = batch_graph()
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.cholesky(p)
    with pytest.raises(MarginalsError) as e:
        g.marginals_joint_any(p, [0], [1])
    assert e.value.code == -12
    p.destroy(); g.destroy()
