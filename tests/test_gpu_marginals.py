"""Marginal covariances on the GPU (aprilsam_amd_marginals / _joint, include/aprilsam_amd.h): selected inversion of the retained factor
(aprilsam_amd/csrc/selinv.hip.h).  Checked against numpy's inverse of the system the step factorised (small and medium graphs), scipy
sparse solves and the matrix-free identity sum_j A_ij Sigma_ji = I (tests/support/marginal_identity.py) at 10^5 and 10^6 poses;
bitwise reproducibility, non-interference with the solver, the incremental path and the error returns."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets, harness
from tests.support.marginal_cases import case_arrays, factor_pairs, tutorial_arrays
from tests.support.marginal_identity import identity_residual
from tests.support.selinv_model import dense_system, sparse_system, system_blocks
from tests.support.sigma_compare import SIG_RTOL, Recorder, compare_dense as _compare_dense, demo_checkpoints

pytestmark = pytest.mark.gpu
# |GPU - reference| / (largest |entry| of the pose's block row of Sigma).  SIG_RTOL = 1e-9 against the dense inverse and its
# calibration on the CPU: tests/support/sigma_compare.py.  splu with two orderings (COLAMD, MMD on A + A') disagrees by 3.4e-10 at K = 120.
SPLU_RTOL = 1e-8         # against splu solves (lattices K = 120, 316): 30 x the K = 120 disagreement of the two CPU references
IDENT_RTOL = 1e-9        # identity residual (relative to the terms it sums)


def _solved(lib, arr, steps=1):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    for _ in range(steps):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
    return g, p


@pytest.mark.parametrize("name", ["tutorial", "random0", "random1", "random2", "random3", "lattice6", "lattice24", "lattice60", "m3500"])
def test_marginals_match_the_dense_inverse(lib, name):
    arr = case_arrays(lib, name)
    g, p = _solved(lib, arr)
    _compare_dense(g, p)
    p.destroy(); g.destroy()


def _identity(g, p, arr):
    states, fa, fb, z, W = arr
    Aii, Aab = system_blocks(g.l_points(), fa, fb, z, W, p.c.tikhanov)
    a, b = factor_pairs(fa, fb)
    jf = np.zeros((len(fa), 6, 6)); jf[fb >= 0] = g.marginals_joint(p, a, b)
    return identity_residual(Aii, Aab, fa, fb, g.marginals(p), jf), Aii, Aab


@pytest.mark.parametrize("K", [120, 316])
def test_lattice_marginals_against_sparse_solves_and_the_identity(lib, K):
    """K = 316 is the 10^5-pose lattice: its separators take the fronts far beyond one workgroup"""
    import scipy.sparse.linalg as sla
    arr = lib.lattice_arrays(K)
    g, p = _solved(lib, arr)
    res, Aii, Aab = _identity(g, p, arr)
    assert res["rel_max"] < IDENT_RTOL, res["rel_max"]
    fa, fb = arr[1], arr[2]
    N = len(arr[0])
    lu = sla.splu(sparse_system(Aii, Aab, fa, fb).tocsc())
    rng = np.random.default_rng(K)
    poses = rng.choice(N, 64, replace=False)
    a, b = factor_pairs(fa, fb)
    pk = rng.choice(len(a), 64, replace=False)
    d = g.marginals(p, poses); j = g.marginals_joint(p, a[pk], b[pk])
    for i, n in enumerate(poses):
        E = np.zeros((3 * N, 3)); E[3 * n:3 * n + 3] = np.eye(3)
        col = lu.solve(E)
        assert np.abs(d[i] - col[3 * n:3 * n + 3]).max() < SPLU_RTOL * np.abs(col).max()
    for i, k in enumerate(pk):
        E = np.zeros((3 * N, 6)); E[3 * a[k]:3 * a[k] + 3, :3] = np.eye(3); E[3 * b[k]:3 * b[k] + 3, 3:] = np.eye(3)
        col = lu.solve(E)
        ref = np.vstack([col[3 * a[k]:3 * a[k] + 3], col[3 * b[k]:3 * b[k] + 3]])
        assert np.abs(j[i] - ref).max() < SPLU_RTOL * np.abs(col).max()
    p.destroy(); g.destroy()


def test_million_pose_lattice_satisfies_the_marginal_identity(lib):
    arr = lib.lattice_arrays(1000)
    g, p = _solved(lib, arr)
    res, _, _ = _identity(g, p, arr)
    assert res["rel_max"] < IDENT_RTOL, res["rel_max"]
    p.destroy(); g.destroy()


def test_two_calls_give_the_same_bits_and_the_second_runs_no_inversion(lib):
    arr = case_arrays(lib, "lattice60")
    g, p = _solved(lib, arr)
    r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    d1 = g.marginals(p)
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0 + 1
    d2 = g.marginals(p)
    a, b = factor_pairs(arr[1], arr[2])
    j1 = g.marginals_joint(p, a, b); j2 = g.marginals_joint(p, a, b)
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0 + 1           # extraction only
    assert d1.tobytes() == d2.tobytes() and j1.tobytes() == j2.tobytes()
    g.cholesky(p)                                                           # a new factor: Sigma again ...
    d3 = g.marginals(p)
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0 + 2
    g2, p2 = _solved(lib, arr, 2)                                           # ... with the same bits as a fresh param's
    assert g2.marginals(p2).tobytes() == d3.tobytes()
    for x in (p, g, p2, g2):
        x.destroy()


def test_batch_steps_are_bitwise_unaffected_by_marginals_calls(lib):
    arr = datasets.random_pose_graph(400, 350, 2)
    runs = []
    for with_m in (False, True):
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        snaps = []
        for _ in range(20):
            g.cholesky(p)
            if with_m:
                g.marginals(p); g.marginals_joint(p, *factor_pairs(arr[1], arr[2]))
            snaps.append(np.concatenate([g.states(), g.deltas(), g.l_points()]).tobytes())
        runs.append(snaps)
        p.destroy(); g.destroy()
    assert runs[0] == runs[1]


def test_params_on_two_slots(lib):
    arr = case_arrays(lib, "lattice24")
    out = []
    for slots in ((0, 0), (0, 1)):
        gs, ps = [], []
        for s in slots:
            g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
            assert lib.dll.aprilsam_amd_param_set_device(p.ptr, s) == 0
            g.cholesky(p); gs.append(g); ps.append(p)
        m = [g.marginals(p) for g, p in zip(gs, ps)]
        for g, p in zip(gs, ps):
            g.cholesky(p)
        out.append([m[0].tobytes(), m[1].tobytes()] + [g.states().tobytes() for g in gs])
        for x in gs + ps:
            x.destroy()
    assert out[0][0] == out[0][1] == out[1][0] == out[1][1]
    assert out[0][2:] == out[1][2:]


def test_incremental_demo_checkpoints_and_non_interference(lib):
    """First 600 steps of the M3500 incremental demo.  Sigma = inv(A(l_point)) with lambda on the poses of the last batch step after
    every batch step (first pose, fall-backs), every re-planned step, the first steps that took low-rank updates of their root path,
    the first loop closures on the fast path, and every 50th step (fast-path steps with tail fronts).  The run's chi^2 trace and
    states are bitwise those of the run without any marginals call."""
    arr = datasets.m3500_arrays()
    plain = harness.run_demo(lib, arr, max_poses=600, record_states_every=50)
    rec = Recorder(lib)
    on_step, seen = demo_checkpoints(rec, arr, lambda g, p, k, lam_nodes: _compare_dense(g, p, lam_nodes), batch_residual=True)
    res = harness.run_demo(rec, arr, max_poses=600, record_states_every=50, on_step=on_step)
    assert seen["batch"] >= 5 and seen["updated"] >= 1 and seen["fast"] >= 12, seen
    assert res["chi2"].tobytes() == plain["chi2"].tobytes()
    assert res["final_states"].tobytes() == plain["final_states"].tobytes()
    for k in plain["snaps"]:
        assert res["snaps"][k].tobytes() == plain["snaps"][k].tobytes()


def test_tutorial_incremental(lib):
    g = lib.new_graph(); p = lib.new_param()
    states, fa, fb, z, W = tutorial_arrays()
    g.add_node_xyt(states[0]); g.add_factor_xytpos(0, z[0], W[0]); g.cholesky(p)
    _compare_dense(g, p)
    for k in range(1, 6):
        g.add_node_xyt(states[k])
        for f in range(1, len(fa)):
            if max(fa[f], fb[f]) == k:
                g.add_factor_xyt(int(fa[f]), int(fb[f]), z[f], W[f])
        p.c.batch_time = 1e300
        g.cholesky_inc(p)
        _compare_dense(g, p, 1)                               # (lambda on the pose of the first batch step only)
    g.cholesky(p)                                             # a batch call on the extended plan (option batch_extend) ...
    _compare_dense(g, p)
    with lib.options(batch_extend=0):                         # ... and on a new plan
        g.cholesky(p)
    _compare_dense(g, p)
    p.destroy(); g.destroy()


def test_after_batch_resident(lib):
    """aprilsam_amd_batch_resident (resident_begin / steps / end): the factor of the LAST iteration, at the l_points resident_end writes"""
    arr = case_arrays(lib, "random1")
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.batch_resident(p, 3)
    assert np.max(np.abs(g.l_points() - arr[0])) > 1e-6          # (not the start: the third iteration's linearisation point)
    _compare_dense(g, p)
    p.destroy(); g.destroy()


def test_joint_pairs_off_the_pattern(lib):
    """pairs not joined on the pattern of L come back all-NaN, whichever of the two is eliminated first, and are counted"""
    from tests.support.mf_emulator import PlanView
    from tests.support.selinv_model import SelInvModel
    arr = case_arrays(lib, "lattice24")
    states, fa, fb, z, W = arr
    N = len(states)
    g, p = _solved(lib, arr)
    Aii, Aab = system_blocks(g.l_points(), fa, fb, z, W, p.c.tikhanov)
    A = dense_system(Aii, Aab, fa, fb)
    Sig = np.linalg.inv(A)
    model = SelInvModel(PlanView(lib, N, fa, fb, xy=states[:, :2]), A)
    rng = np.random.default_rng(5)
    a = rng.integers(0, N, 400); b = rng.integers(0, N, 400)
    keep = a != b
    a, b = a[keep].astype(np.int32), b[keep].astype(np.int32)
    off = np.isnan(model.joint(a, b)).all(axis=(1, 2))
    pos = model.pos
    assert (off & (pos[a] < pos[b])).any() and (off & (pos[a] > pos[b])).any() and (~off).any()
    out = np.empty((len(a), 6, 6))
    rc = lib.dll.aprilsam_amd_marginals_joint(g.ptr, p.ptr, len(a), a.ctypes.data_as(C.POINTER(C.c_int)), b.ctypes.data_as(C.POINTER(C.c_int)),
                                              out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == int(off.sum())
    assert np.isnan(out[off]).all() and not np.isnan(out[~off]).any()
    scale = np.abs(Sig).max()
    for k in np.nonzero(~off)[0]:
        ix = np.r_[3 * a[k]:3 * a[k] + 3, 3 * b[k]:3 * b[k] + 3]
        assert np.abs(out[k] - Sig[np.ix_(ix, ix)]).max() < SIG_RTOL * scale
    p.destroy(); g.destroy()


def test_sharded_param_is_refused(lib):
    from aprilsam_amd.host import MarginalsError
    arr = case_arrays(lib, "lattice24")
    g, p = _solved(lib, arr)
    d = lib.dll
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]     # (as aprilsam_amd/shard.py binds them)
    d.aprilsam_amd_shard_end.argtypes = [C.c_void_p]
    gp, pp = C.cast(g.ptr, C.c_void_p), C.cast(p.ptr, C.c_void_p)
    assert d.aprilsam_amd_shard_begin(gp, pp, 0, 1) == 0             # (one rank of one: the state a sharded run starts from)
    with pytest.raises(MarginalsError) as e:
        g.marginals(p)
    assert e.value.code == -12
    d.aprilsam_amd_shard_end(pp)
    p.destroy(); g.destroy()


def test_error_returns_leave_the_solver_untouched(lib):
    from aprilsam_amd.host import MarginalsError
    arr = case_arrays(lib, "lattice60")
    ref_g, ref_p = _solved(lib, arr, 2)
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    with pytest.raises(MarginalsError) as e:                  # never solved
        g.marginals(p)
    assert e.value.code == -1 and lib.last_error()[0] == -1
    g.cholesky(p)
    with pytest.raises(MarginalsError) as e:                  # a node id out of range
        g.marginals(p, [len(arr[0])])
    assert e.value.code == -13
    with pytest.raises(MarginalsError) as e:
        g.marginals_joint(p, [0], [-1])
    assert e.value.code == -13
    lib.set_option("mem_cap_mb", 1)                           # the Sigma pool refused: -11
    try:
        with pytest.raises(MarginalsError) as e:
            g.marginals(p)
        assert e.value.code == -11
    finally:
        lib.set_option("mem_cap_mb", 0)
    g.cholesky(p)
    assert g.states().tobytes() == ref_g.states().tobytes()   # the next solver call: the same bits
    assert g.marginals(p).tobytes() == ref_g.marginals(ref_p).tobytes()
    n = g.n_nodes                                             # nodes added since the last solve
    g.add_node_xyt([0.5, 0.5, 0.0]); g.add_factor_xyt(n - 1, n, [0.1, 0, 0], np.eye(3) * 10)
    with pytest.raises(MarginalsError) as e:
        g.marginals(p)
    assert e.value.code == -13
    assert g.marginals(p, [0, n - 1]).shape == (2, 3, 3)
    for x in (p, g, ref_p, ref_g):
        x.destroy()


def test_asymmetric_information_is_refused(lib):
    from aprilsam_amd.host import MarginalsError
    from tests.support.asym_scenarios import batch_graph
    arr = batch_graph()
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.cholesky(p)
    before = g.states().tobytes()
    with pytest.raises(MarginalsError) as e:
        g.marginals(p)
    assert e.value.code == -12
    g2 = lib.new_graph(); g2.build_from_arrays(*arr); p2 = lib.new_param()
    g2.cholesky(p2); g2.cholesky(p2); g.cholesky(p)
    assert before != g.states().tobytes() and g.states().tobytes() == g2.states().tobytes()
    for x in (p, g, p2, g2):
        x.destroy()
