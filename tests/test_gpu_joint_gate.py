"""aprilsam_amd_marginals_set and aprilsam_amd_gate_xyt_joint on the GPU (aprilsam_amd/csrc/jointgate.hip.h): the dense
joint covariance of a node set against numpy's inverse of the factorised system and bit for bit against aprilsam_amd_marginals_joint_any;
the joint compatibility gate against the numpy model (tests/support/joint_gate_model.py), its prefix, repeatability and permutation
properties, the open-chain scenario, fixed nodes, the M3500 incremental demo, non-interference and every refusal.  The path solves below
the new kernel are held to every kernel path and launch form by tests/test_gpu_consumer_paths.py / test_gpu_consumer_inc.py."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets, harness
from aprilsam_amd.host import MarginalsError
from tests.support.consumer_graphs import two_components
from tests.support.gate_model import CHI2_3_999, gate, predict
from tests.support.joint_gate_model import dense_sigma, dense_tolerances, joint_gate, set_cov
from tests.support.marginal_cases import case_arrays
from tests.support.mf_emulator import PlanView
from tests.support.sigma_compare import SIG_RTOL, Recorder, demo_checkpoints, dense as _dense, ref_joint
from tests.test_gpu_gating import GATE_RTOL
from tests.test_joint_gate_model import chain_scenario, chi2_quantile

pytestmark = pytest.mark.gpu
SENT = -7.0
W0 = np.diag([100.0, 100.0, 400.0]).ravel()


def _solved(lib, arr, steps=1, fixed=()):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    for i in fixed:
        assert g.set_fixed(int(i)) == 0
    for _ in range(steps):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
    return g, p


def _sigma(g, p, lam_nodes=None, fixed=()):
    return dense_sigma(g.l_points(), *g.arrays()[1:], p.c.tikhanov, lam_nodes, fixed)


def _check_set(g, p, nodes, Sig, scale):
    """marginals_set of `nodes`: against the dense inverse to SIG_RTOL, exactly symmetric, its blocks bitwise joint_any's S_ab"""
    nodes = np.asarray(nodes, np.int32)
    k = len(nodes)
    M = g.marginals_set(p, nodes)
    assert M.shape == (3 * k, 3 * k) and np.isfinite(M).all() and np.array_equal(M, M.T)
    sc = np.repeat(scale[nodes], 3)
    err = (np.abs(M - set_cov(Sig, nodes)) / np.maximum(sc[:, None], sc[None, :])).max()
    assert err < SIG_RTOL, (nodes, err)
    ia, ib = np.repeat(np.arange(k), k), np.tile(np.arange(k), k)
    J = g.marginals_joint_any(p, nodes[ia], nodes[ib])
    blocks = M.reshape(k, 3, k, 3).transpose(0, 2, 1, 3).reshape(k * k, 3, 3)
    assert blocks.tobytes() == np.ascontiguousarray(J[:, :3, 3:]).tobytes(), nodes
    return M


@pytest.mark.parametrize("name", ["tutorial", "random0", "random1", "random2", "random3", "lattice12"])
def test_marginals_set_matches_the_dense_inverse_and_joint_any(lib, name):
    arr = case_arrays(lib, name)
    g, p = _solved(lib, arr)
    N = len(arr[0])
    Sig, scale = _dense(g, p)
    rng = np.random.default_rng(5)
    for k in (1, 2, 7, 33):                                     # (33 > N on the small graphs: nodes repeat)
        _check_set(g, p, rng.choice(N, k, replace=k > N), Sig, scale)
    P = PlanView(lib, N, arr[1], arr[2], xy=arr[0][:, :2])
    t = int(np.argmax(P.front_nsb))                             # within one front
    _check_set(g, p, P.perm[P.front_first[t]:P.front_first[t] + P.front_nsb[t]][:6], Sig, scale)
    leaves = np.setdiff1d(np.arange(P.nF), P.front_parent[P.front_parent >= 0])[:6]      # one node of each of six leaves: different subtrees
    _check_set(g, p, P.perm[P.front_first[leaves]], Sig, scale)
    M = _check_set(g, p, [N - 1, 0, N - 1, 1 % N, 0], Sig, scale)           # duplicates: the blocks repeat
    assert M[:3].tobytes() == M[6:9].tobytes() and M[3:6].tobytes() == M[12:].tobytes()
    cov = np.full(9, SENT)                                      # k = 0: 0, nothing written
    assert lib.dll.aprilsam_amd_marginals_set(g.ptr, p.ptr, 0, None, cov.ctypes.data_as(C.POINTER(C.c_double))) == 0 and np.all(cov == SENT)
    assert g.marginals_set(p, []).shape == (0, 0)
    p.destroy(); g.destroy()


def test_marginals_set_across_components_is_exactly_zero(lib):
    arr, comp = two_components()
    g, p = _solved(lib, arr)
    Sig, scale = _dense(g, p)
    n0 = np.nonzero(comp == 0)[0]; n1 = np.nonzero(comp == 1)[0]
    nodes = np.r_[n0[[0, 7, 200]], n1[[3, 50]], n0[399], n1[3]].astype(np.int32)
    M = _check_set(g, p, nodes, Sig, scale)
    cross = comp[nodes][:, None] != comp[nodes][None, :]
    blk = M.reshape(len(nodes), 3, len(nodes), 3).transpose(0, 2, 1, 3)
    assert cross.any() and blk[cross].tobytes() == np.zeros_like(blk[cross]).tobytes()
    p.destroy(); g.destroy()


# ---- the gate ------------------------------------------------------------------------------------------------------------------------
def _device_sigma(g, p, hyps):
    """the model's Sigma from the DEVICE's blocks of the nodes the hypotheses name (zero elsewhere: the model reads nothing else)"""
    nodes = np.unique(np.concatenate([np.r_[h[0], h[1]] for h in hyps])).astype(np.int32)
    M = g.marginals_set(p, nodes)
    Sig = np.zeros((3 * g.n_nodes, 3 * g.n_nodes))
    ix = (3 * nodes[:, None] + np.arange(3)).ravel()
    Sig[np.ix_(ix, ix)] = M
    return Sig


def _candidates(st, a, b, seed, noise=0.3):
    """z near the prediction at the states st, W random symmetric positive definite"""
    rng = np.random.default_rng(seed)
    n = len(a)
    z = np.array([predict(st[i], st[j]) for i, j in zip(a, b)]) + rng.normal(size=(n, 3)) * noise
    L = rng.normal(size=(n, 3, 3)) * 0.3 + np.eye(3) * 3
    return np.asarray(a, np.int32), np.asarray(b, np.int32), z, np.einsum("nij,nkj->nik", L, L).reshape(n, 9)


def _check_hyps(g, p, st, hyps, d2, Cs, dense):
    """the device's Sigma of the hypotheses' nodes against the dense inverse `dense` (SIG_RTOL); the gate against the model on the device's
    Sigma (GATE_RTOL) and on the dense inverse (what SIG_RTOL allows: joint_gate_model.dense_tolerances).  Returns the worst d2 error"""
    Sig = _device_sigma(g, p, hyps)
    nodes = np.unique(np.concatenate([np.r_[h[0], h[1]] for h in hyps]))
    sc = np.repeat(np.abs(dense).reshape(len(st), 3, -1).max(axis=(1, 2))[nodes], 3)
    sc = np.maximum(sc[:, None], sc[None, :])
    err = np.abs(set_cov(Sig, nodes) - set_cov(dense, nodes)) / np.where(sc > 0, sc, 1.0)
    assert err.max() < SIG_RTOL, err.max()
    worst = 0.0
    for h, d, Cm in zip(hyps, d2, Cs):
        pre, Cw, _ = joint_gate(st, *h, Sig)
        assert (np.abs(d - pre) <= GATE_RTOL * np.abs(pre)).all(), (d, pre)
        assert np.abs(Cm - Cw).max() < GATE_RTOL * np.abs(Cw).max() and np.array_equal(Cm, Cm.T)
        worst = max(worst, (np.abs(d - pre) / pre).max())
        pre, Cw, _ = joint_gate(st, *h, dense)
        rtol, c_atol = dense_tolerances(st, h[0], h[1], h[2], Cw, dense, SIG_RTOL)
        assert (np.abs(d - pre) <= rtol * pre).all() and np.abs(Cm - Cw).max() <= c_atol, (d, pre, rtol, c_atol)
    return worst


def _cut(h, k):
    return tuple(x[k] for x in h)


@pytest.fixture(scope="module")
def scene(lib):
    """random2 (400 poses) after two steps; one call that mixes hypotheses of m = 1, 2, 3, 5 and 16 on a pool of ten poses (candidates share
    nodes; the m = 5 one repeats a pair and holds a pair as (a, b) and as (b, a)), then the 16's first j candidates for every j < 16"""
    arr = case_arrays(lib, "random2")
    g, p = _solved(lib, arr, 2)
    st = g.states()
    rng = np.random.default_rng(8)
    pool = rng.choice(len(st), 10, replace=False)
    ia = rng.integers(0, 10, 27)
    a = pool[ia]; b = pool[(ia + rng.integers(1, 10, 27)) % 10]
    a[8], b[8] = a[6], b[6]                                     # (6..10 is the m = 5 hypothesis) the pair of 6 again
    a[10], b[10] = b[7], a[7]                                   # the pair of 7 the other way round
    cand = _candidates(st, a, b, 9)
    cuts = [slice(0, 1), slice(1, 3), slice(3, 6), slice(6, 11), slice(11, 27)]
    hyps = [_cut(cand, k) for k in cuts]
    hyps += [_cut(hyps[4], slice(0, j)) for j in range(1, 16)]
    bad, d2, Cs = g.gate_xyt_joint(p, hyps)
    yield dict(lib=lib, g=g, p=p, st=st, hyps=hyps, bad=bad, d2=d2, C=Cs)
    p.destroy(); g.destroy()


def test_gate_joint_matches_the_model(scene):
    g, p, hyps = scene["g"], scene["p"], scene["hyps"][:5]
    assert scene["bad"] == 0 and [len(h[0]) for h in hyps] == [1, 2, 3, 5, 16]
    worst = _check_hyps(g, p, scene["st"], hyps, scene["d2"], scene["C"], _sigma(g, p))
    print(f"worst relative d2 error against the model on the device's Sigma: {worst:.2e}")


def test_one_candidate_agrees_with_gate_xyt(scene):
    g, p = scene["g"], scene["p"]
    cand = tuple(np.concatenate([h[k] for h in scene["hyps"][:5]]) for k in range(4))
    d2, S = g.gate_xyt(p, *cand)
    bad, jd2, jC = g.gate_xyt_joint(p, [_cut(cand, slice(i, i + 1)) for i in range(len(d2))])
    assert bad == 0
    for i in range(len(d2)):
        assert abs(jd2[i][0] - d2[i]) <= GATE_RTOL * d2[i] and np.abs(jC[i] - S[i]).max() <= GATE_RTOL * np.abs(S[i]).max(), i


def test_truncated_hypotheses_reproduce_the_prefixes_bit_for_bit(scene):
    full_d2, full_C = scene["d2"][4], scene["C"][4]
    for j in range(1, 16):
        d2, Cm = scene["d2"][4 + j], scene["C"][4 + j]
        assert d2.tobytes() == full_d2[:j].tobytes(), j
        assert Cm.tobytes() == np.ascontiguousarray(full_C[:3 * j, :3 * j]).tobytes(), j


def test_two_calls_give_the_same_bits_and_the_total_is_permutation_invariant(scene):
    g, p, hyps = scene["g"], scene["p"], scene["hyps"]
    bad, d2, Cs = g.gate_xyt_joint(p, hyps)
    assert bad == 0
    for x, y in zip(d2 + Cs, scene["d2"] + scene["C"]):
        assert x.tobytes() == y.tobytes()
    rng = np.random.default_rng(2)
    perm = [_cut(hyps[4], rng.permutation(16)) for _ in range(4)] + [_cut(hyps[3], rng.permutation(5))]
    _, pd2, _ = g.gate_xyt_joint(p, perm)
    for k, d in enumerate(pd2):
        tot = scene["d2"][4 if k < 4 else 3][-1]
        assert abs(d[-1] - tot) <= GATE_RTOL * tot, (k, d[-1], tot)


def test_a_call_that_names_more_than_1024_nodes(lib):
    """the driver keeps its pair codes in a dense table up to 1024 distinct nodes and in a hash map beyond (PairBook, solver_gating.inc.h):
    350 hypotheses of two candidates on 1400 distinct poses give, each, the bits of the call that sends it alone"""
    arr = case_arrays(lib, "random3")
    g, p = _solved(lib, arr, 2)
    st = g.states()
    nodes = np.random.default_rng(6).permutation(len(st))[:1400].reshape(350, 4)
    hyps = [_candidates(st, q[[0, 2]], q[[1, 3]], k) for k, q in enumerate(nodes)]
    bad, d2, Cs = g.gate_xyt_joint(p, hyps)
    assert bad == 0
    for k in range(0, 350, 17):
        _, d1, C1 = g.gate_xyt_joint(p, [hyps[k]])
        assert d1[0].tobytes() == d2[k].tobytes() and C1[0].tobytes() == Cs[k].tobytes(), k
    _check_hyps(g, p, st, hyps[:3], d2[:3], Cs[:3], _sigma(g, p))
    p.destroy(); g.destroy()


def test_chain_scenario_decides_as_the_cpu_model(lib):
    arr, a, b, z, W = chain_scenario()
    g, p = _solved(lib, arr)
    single, _ = g.gate_xyt(p, a, b, z, W)
    bad, d2, Cs = g.gate_xyt_joint(p, [(a, b, z, W)])
    Sig = _sigma(g, p)
    pre, Cw, _ = joint_gate(g.states(), a, b, z, W, Sig)
    msingle, _ = gate(g.states(), a, b, z, W, ref_joint(Sig, a, b))
    gates = np.array([CHI2_3_999, chi2_quantile(6)])
    print(f"single {single}, joint prefixes {d2[0]} (model {pre}), gates {gates}")
    assert bad == 0 and np.array_equal(single < CHI2_3_999, msingle < CHI2_3_999) and (single < CHI2_3_999).all()
    assert np.array_equal(d2[0] < gates, pre < gates) and d2[0][0] < gates[0] and d2[0][1] > gates[1]
    _check_hyps(g, p, g.states(), [(a, b, z, W)], d2, Cs, Sig)
    p.destroy(); g.destroy()


def test_fixed_node_enters_with_zero_covariance(lib):
    arr = case_arrays(lib, "random1")
    g, p = _solved(lib, arr, 1, fixed=(0,))
    st = g.states()
    hyps = [_candidates(st, [0, 7, 5, 30], [5, 0, 7, 0], 3), _candidates(st, [0], [41], 4), _candidates(st, [12, 41], [41, 5], 5)]
    bad, d2, Cs = g.gate_xyt_joint(p, hyps)
    assert bad == 0
    Sig = _sigma(g, p, fixed=(0,))
    M = g.marginals_set(p, [5, 0, 41])
    assert M[3:6].tobytes() == np.zeros((3, 9)).tobytes() and M[:, 3:6].tobytes() == np.zeros((9, 3)).tobytes()
    _check_hyps(g, p, st, hyps, d2, Cs, Sig)
    Wi = np.linalg.inv(hyps[1][3][0].reshape(3, 3))             # (one fixed end: only the free pose's covariance enters)
    assert np.abs(Cs[1] - Wi).max() > 1e-6
    p.destroy(); g.destroy()


def test_incremental_demo_checkpoints_and_non_interference(lib):
    """First 300 steps of the M3500 incremental demo: at every checkpoint one 5-candidate hypothesis from the newest pose to old poses
    against the model on the dense inverse (lambda on the poses of the last batch step); chi^2 trace and states bitwise those of the run
    without the calls"""
    arr = datasets.m3500_arrays()
    plain = harness.run_demo(lib, arr, max_poses=300, record_states_every=50)
    rec = Recorder(lib)
    worst = [0.0, 0]

    def check(g, p, k, lam_nodes):
        N = g.n_nodes
        if N < 6:
            return
        st = g.states()
        h = _candidates(st, np.full(5, N - 1), np.linspace(0, N - 2, 5).astype(int), k, 0.05)
        h = (h[0], h[1], h[2], np.tile(W0, (5, 1)))
        bad, d2, Cs = g.gate_xyt_joint(p, [h])
        assert bad == 0
        worst[0] = max(worst[0], _check_hyps(g, p, st, [h], d2, Cs, _sigma(g, p, lam_nodes))); worst[1] += 1
    on_step, seen = demo_checkpoints(rec, arr, check)
    res = harness.run_demo(rec, arr, max_poses=300, record_states_every=50, on_step=on_step)
    print(f"{worst[1]} checkpoints {seen}: worst relative d2 error against the model on the device's Sigma {worst[0]:.2e}")
    assert seen["batch"] >= 1 and worst[1] >= 5, seen
    assert res["chi2"].tobytes() == plain["chi2"].tobytes()
    assert res["final_states"].tobytes() == plain["final_states"].tobytes()
    for k in plain["snaps"]:
        assert res["snaps"][k].tobytes() == plain["snaps"][k].tobytes()


def test_batch_steps_are_bitwise_unaffected(lib):
    arr = datasets.random_pose_graph(400, 350, 2)
    runs = []
    for with_calls in (False, True):
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        snaps = []
        for it in range(4):
            g.cholesky(p)
            if with_calls:
                r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
                g.gate_xyt_joint(p, [_candidates(g.states(), [3, 100, 399], [250, 3, 7], it)]); g.marginals_set(p, [5, 399, 17, 5])
                assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0
            snaps.append(np.concatenate([g.states(), g.deltas(), g.l_points()]).tobytes())
        runs.append(snaps)
        p.destroy(); g.destroy()
    assert runs[0] == runs[1]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(lib, g, p, ptr, a, b, z=None, W=None):
    """one raw call on sentinel-filled outputs; a refusal must leave them untouched and record its code"""
    ptr = np.asarray(ptr, np.int32); a = np.asarray(a, np.int32); b = np.asarray(b, np.int32)
    n = len(a)
    z = np.zeros((n, 3)) if z is None else np.ascontiguousarray(z, float)
    W = np.tile(W0, (n, 1)) if W is None else np.ascontiguousarray(W, float)
    d2 = np.full(n + 1, SENT); Cm = np.full(9 * n * n + 1, SENT)
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int)
    lib.clear_error()
    rc = lib.dll.aprilsam_amd_gate_xyt_joint(g.ptr, p.ptr, len(ptr) - 1, ptr.ctypes.data_as(ip), a.ctypes.data_as(ip), b.ctypes.data_as(ip),
                                             z.ctypes.data_as(dp), W.ctypes.data_as(dp), d2.ctypes.data_as(dp), Cm.ctypes.data_as(dp))
    if rc < 0:
        assert np.all(d2 == SENT) and np.all(Cm == SENT) and lib.last_error()[0] == rc
    return rc


def test_refusals_write_nothing_and_leave_the_factor(lib):
    arr = case_arrays(lib, "lattice24")
    N = len(arr[0])
    ref_g, ref_p = _solved(lib, arr, 2)
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    assert _raw(lib, g, p, [0, 2], [0, 5], [9, 7]) == -1                                  # before any solve
    with pytest.raises(MarginalsError) as e:
        g.marginals_set(p, [0, 1])
    assert e.value.code == -1
    g.cholesky(p)
    r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    assert _raw(lib, g, p, [0, 2], [0, 5], [9, 7]) == 0
    assert _raw(lib, g, p, [0, 17], np.arange(17), np.arange(17) + 20) == -13             # 17 candidates
    assert _raw(lib, g, p, [0, 16], np.arange(16), np.arange(16) + 20) == 0
    assert _raw(lib, g, p, [0, 1, 1, 2], [0, 5], [9, 7]) == -13                           # an empty hypothesis
    assert _raw(lib, g, p, [0, 2, 1], [0, 5], [9, 7]) == -13                              # hyp_ptr decreases
    assert _raw(lib, g, p, [1, 2], [0, 5], [9, 7]) == -13                                 # hyp_ptr does not start at 0
    assert _raw(lib, g, p, [0, 2], [0, 5], [9, 5]) == -13                                 # a == b
    z = np.zeros((2, 3)); z[1, 0] = np.nan
    assert _raw(lib, g, p, [0, 2], [0, 5], [9, 7], z=z) == -13
    W = np.tile(W0, (2, 1)); W[1] = np.diag([1.0, -1.0, 1.0]).ravel()
    assert _raw(lib, g, p, [0, 2], [0, 5], [9, 7], W=W) == -12                            # an indefinite W
    assert _raw(lib, g, p, [0, 2], [0, 5], [9, N]) == -13 and _raw(lib, g, p, [0, 2], [0, -1], [9, 7]) == -13      # beyond the system
    assert _raw(lib, g, p, [0], [], []) == 0                                              # n_hyp == 0
    for nodes in ([0, N], [-1]):
        cov = np.full(36, SENT); idx = np.array(nodes, np.int32)
        assert lib.dll.aprilsam_amd_marginals_set(g.ptr, p.ptr, len(idx), idx.ctypes.data_as(C.POINTER(C.c_int)), cov.ctypes.data_as(C.POINTER(C.c_double))) == -13
        assert np.all(cov == SENT)
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0
    g.cholesky(p)                                                                         # the next solver call: the same bits
    assert g.states().tobytes() == ref_g.states().tobytes()
    assert g.marginals_set(p, [3, 80, 3, 500]).tobytes() == ref_g.marginals_set(ref_p, [3, 80, 3, 500]).tobytes()
    d = lib.dll
    assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0                               # a resident run in progress
    assert _raw(lib, g, p, [0, 2], [0, 5], [9, 7]) == -1
    d.aprilsam_amd_resident_end(g.ptr, p.ptr)
    g.cholesky(p)
    assert _raw(lib, g, p, [0, 2], [0, 5], [9, 7]) == 0
    g.optimize_lm(p, max_iters=2)                                                         # LM drops the factor
    assert _raw(lib, g, p, [0, 2], [0, 5], [9, 7]) == -1
    with pytest.raises(MarginalsError) as e:
        g.marginals_set(p, [0, 1])
    assert e.value.code == -1
    for x in (p, g, ref_p, ref_g):
        x.destroy()
