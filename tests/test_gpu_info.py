"""aprilsam_amd_logdet, aprilsam_amd_logdet_sets and aprilsam_amd_info_gain_xyt on the GPU (aprilsam_amd/csrc/infomeasure.hip.h, DESIGN.md
section 32) against the numpy model (tests/support/info_model.py, pinned on the CPU by tests/test_info_model.py): the whole-system
log-determinant after batch and incremental steps, behind every kernel path, on every designed front shape and around the chunk width of
k_logdet_partial, with fixed nodes; set prefixes and gain prefixes against the model on the device's own Sigma blocks (tight) and on the
dense inverse (loose), their bitwise prefix property, what they mean end to end; non-interference and every refusal.

Every tolerance is derived in info_model from the dense system (its module docstring); each family prints its largest error and the ratio
to its bound."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets
from aprilsam_amd.host import MarginalsError
from tests.support import clique_trees as CT
from tests.support import inc_designs as ID
from tests.support import info_model as IM
from tests.support import retained_contract as rc
from tests.support.consumer_graphs import two_components
from tests.support.gate_model import predict
from tests.support.joint_gate_model import dense_sigma
from tests.support.kernel_paths import KERNEL_PATHS
from tests.support.marginal_cases import case_arrays
from tests.support.mf_emulator import PlanView
from tests.support.sigma_compare import SIG_RTOL

pytestmark = pytest.mark.gpu
SENT = -7.0
CHUNK = 768                      # LD_CHUNK of infomeasure.hip.h: own columns per wave of k_logdet_partial
# tests/test_gpu_consumer_paths.py: the option sets beyond KERNEL_PATHS, those whose outputs are bitwise the default's, those that change the tree
EXTRA_PATHS = [dict(pool_guard=64), dict(pool_guard=64, small_lds_kb=0), dict(xcd_place=0), dict(amalg=1), dict(pool_poison=1)]
BITWISE = [dict(pool_guard=64), dict(xcd_place=0), dict(pool_poison=1)]
CHANGES_THE_TREE = ("leaf_nodes", "pin_last", "amalg")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _solved(lib, arr, steps=1, fixed=()):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    for i in fixed:
        assert g.set_fixed(int(i)) == 0
    for _ in range(steps):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
    return g, p


def _A(g, p, lam_nodes=None):
    return IM.system_matrix(g.l_points(), *g.arrays()[1:], p.c.tikhanov, lam_nodes)


def _check_logdet(g, p, what, A=None, fixed=(), tol=None):
    """logdet against the model on A (default: the graph's system at its l_points); two calls give the same bits.  Returns (value, error, bound)"""
    A = _A(g, p) if A is None else A
    got = g.logdet(p)
    assert np.float64(got).tobytes() == np.float64(g.logdet(p)).tobytes()
    ref = IM.logdet(A, fixed)
    tol = IM.logdet_tolerance(A, fixed) if tol is None else tol
    err = abs(got - ref)
    print(f"[logdet] {what}: {got:.12g} (model {ref:.12g}), error {err:.2e}, bound {tol:.2e}, ratio {err / tol:.3f}")
    assert np.isfinite(got) and err <= tol, (what, got, ref, err, tol)
    return got, err, tol


# ---- 1. logdet against the dense model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tutorial", "random0", "random1", "random2", "random3", "lattice12"])
def test_logdet_matches_the_dense_model_after_one_and_two_steps(lib, name):
    arr = case_arrays(lib, name)
    g, p = _solved(lib, arr, 0)
    for step in (1, 2):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
        r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
        _check_logdet(g, p, f"{name}, step {step}")
        assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0
    p.destroy(); g.destroy()


# ---- 2. behind every option set ------------------------------------------------------------------------------------------------------------
ARR700 = datasets.random_pose_graph(700, 600, 21)


def _logdet700(lib, opts):
    with lib.options(**opts):
        g, p = _solved(lib, ARR700, 2)
        got, ref, nf = g.logdet(p), IM.logdet(_A(g, p)), p.stats()["n_fronts"]
        p.destroy(); g.destroy()
    return got, ref, nf


@pytest.fixture(scope="module")
def default700(lib):
    g, p = _solved(lib, ARR700, 2)
    tol = IM.logdet_tolerance(_A(g, p))
    p.destroy(); g.destroy()
    return _logdet700(lib, {}) + (tol,)


@pytest.mark.parametrize("opts", KERNEL_PATHS + EXTRA_PATHS, ids=_ids)
def test_logdet_behind_every_kernel_path(lib, default700, opts):
    base, _, base_nf, tol = default700
    got, ref, nf = _logdet700(lib, opts)
    print(f"[logdet] {_ids(opts)}: error {abs(got - ref):.2e}, bound {tol:.2e}, ratio {abs(got - ref) / tol:.3f}; against the default run {abs(got - base):.2e}")
    assert abs(got - ref) <= tol, (opts, got, ref)
    if opts in BITWISE:
        assert np.float64(got).tobytes() == np.float64(base).tobytes(), (opts, got, base)
    if any(k in opts for k in CHANGES_THE_TREE):                 # (another elimination order: the same determinant)
        assert nf != base_nf and abs(got - base) <= 2 * tol, (opts, got, base)


# ---- 3. every designed front shape, the chunk width, the wide root ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CT.CASES))
def test_logdet_on_every_designed_front_shape(lib, name):
    levels, fan, designed, _ = CT.CASES[name]
    arr = CT.clique_tree(levels, fan, CT.SEED)
    g, p = _solved(lib, arr)
    _check_logdet(g, p, name)
    p.destroy(); g.destroy()


@pytest.mark.parametrize("n", [CHUNK // 3 - 1, CHUNK // 3, CHUNK // 3 + 1, 2 * CHUNK // 3, 2 * CHUNK // 3 + 1])
def test_logdet_around_the_chunk_width(lib, n):
    """one front whose own columns are chunk - 3, chunk, chunk + 3 (one chunk; a whole number of chunks; one column block over), two chunks
    and two chunks + 3"""
    arr = CT.clique_tree((n,), 1, CT.SEED)
    P = PlanView(lib, n, arr[1], arr[2], xy=arr[0][:, :2])
    assert P.nF == 1 and int(P.front_nsb[0]) == n
    g, p = _solved(lib, arr)
    _check_logdet(g, p, f"one front of {3 * n} own columns (chunk {CHUNK})")
    p.destroy(); g.destroy()


def test_logdet_on_the_wide_root_ending_in_a_partial_outer_block(lib):
    arr = datasets.random_pose_graph(3000, 1800, 102)            # (tests/test_gpu_consumer_paths.py: ARR3000, its root front of 645 poses)
    g, p = _solved(lib, arr)
    assert p.stats()["max_front_rows"] > 1900
    _check_logdet(g, p, "random 3000 / 1800 / 102")
    p.destroy(); g.destroy()


# ---- 4. after incremental steps ----------------------------------------------------------------------------------------------------------------
INC_SCENARIOS = ["tail steps, tail_poses = 8", "6,5,5 x2: a mid front"]


def test_logdet_after_incremental_steps_of_every_form(lib):
    """designed incremental runs (tests/support/inc_designs.py): after every april_graph_cholesky_inc -- the primer's re-plan, fast tail
    steps, general steps with low-rank updates, and a last call forced to fall back to a batch step -- logdet against the model on the exact
    system of that step (tests/support/inc_exact.py: incremental_system)"""
    seen = {}
    for name in INC_SCENARIOS:
        B, sc = ID.build(name), ID.SCENARIOS[name]
        o = {k: sc[k] for k in ("tail_poses", "small_threads") if sc[k]}
        with lib.options(**o):
            g = lib.new_graph(); g.build_from_arrays(*B["base"])
            p = lib.new_param(nthreshold=10 ** 6, delta_xy=ID.DELTA_XY, delta_theta=ID.DELTA_THETA)
            g.cholesky(p)
            _check_logdet(g, p, f"{name}: the batch step")
            fa, fb, z, W = (np.array(x) for x in B["base"][1:])
            q = np.where((fb < 0)[:, None], g.l_points()[fa], 0.0)
            n_batch = g.n_nodes
            for k, (st, nfa, nfb, nz, nW, ok) in enumerate(B["calls"]):
                last = k == len(B["calls"]) - 1
                for s in st:
                    g.add_node_xyt(s)
                now = g.states()
                for a, b, zz, WW in zip(nfa, nfb, nz, nW):
                    if b >= 0:
                        g.add_factor_xyt(int(a), int(b), zz, WW.reshape(3, 3))
                    else:
                        g.add_factor_xytpos(int(a), zz, WW.reshape(3, 3))
                fa = np.r_[fa, nfa].astype(np.int32); fb = np.r_[fb, nfb].astype(np.int32); z = np.vstack([z, nz]); W = np.vstack([W, nW])
                q = np.vstack([q, np.where((nfb < 0)[:, None], now[nfa], 0.0).reshape(-1, 3)])
                p.c.batch_time = 1e300                           # (the wall-clock rule of the reference never fires)
                if last:
                    p.c.nthreshold = -1                          # every count of relinearised poses exceeds it: the call ends in a batch step
                bt = p.c.batch_time
                g.cholesky_inc(p)
                stats = p.stats()
                assert stats["not_spd"] == 0 and stats["error_code"] == 0, (name, k, stats)
                head, rows = p.inc_forms()
                fell_back = p.c.batch_time != bt
                assert fell_back == last, (name, k)
                if fell_back:
                    form, n_batch = "batch fall-back", g.n_nodes
                    q = np.where((fb < 0)[:, None], g.l_points()[fa], 0.0)
                else:
                    form = "re-plan" if head["path"] == "re-plan" else "low-rank update" if stats["inc_fronts_updated"] > 0 else head["path"]
                seen[form] = seen.get(form, 0) + 1
                A = IM.incremental_matrix(g.l_points(), fa, fb, z, W, q, n_batch, p.c.tikhanov)
                _check_logdet(g, p, f"{name}: call {k} ({form}, {g.n_nodes} poses)", A=A)
            p.destroy(); g.destroy()
    print(f"[logdet] forms taken: {seen}")
    assert seen.get("re-plan", 0) >= 1 and seen.get("low-rank update", 0) >= 1 and seen.get("batch fall-back", 0) >= 1
    assert any(k.startswith("tail") for k in seen), seen


# ---- 5. fixed nodes ------------------------------------------------------------------------------------------------------------------------------
def _candidates(st, a, b, seed):
    rng = np.random.default_rng(seed)
    n = len(a)
    L = rng.normal(size=(n, 3, 3)) * 0.3 + np.eye(3) * 3
    return np.asarray(a, np.int32), np.asarray(b, np.int32), np.einsum("nij,nkj->nik", L, L).reshape(n, 9)


def _device_sigma(g, p, nodes):
    """the model's Sigma from the DEVICE's blocks of `nodes` (zero elsewhere: the model reads nothing else)"""
    nodes = np.unique(np.asarray(nodes)).astype(np.int32)
    M = g.marginals_set(p, nodes)
    Sig = np.zeros((3 * g.n_nodes, 3 * g.n_nodes))
    ix = (3 * nodes[:, None] + np.arange(3)).ravel()
    Sig[np.ix_(ix, ix)] = M
    return Sig


def _check_gain(g, p, st, hyps, gains, dense, what):
    """every prefix against the model on the device's own Sigma (tight) and on the dense inverse (loose); >= 0 and non-decreasing"""
    worst = [0.0, 0.0]
    for h, got in zip(hyps, gains):
        a, b, W = h
        Sig = _device_sigma(g, p, np.r_[a, b])
        ref, tol = IM.gain_prefixes(st, a, b, W, Sig), IM.gain_tight_tolerance(st, a, b, W, Sig)
        assert (np.abs(got - ref) <= tol).all(), (what, got, ref, tol)
        worst[0] = max(worst[0], (np.abs(got - ref) / tol).max())
        ref, tol = IM.gain_prefixes(st, a, b, W, dense), IM.gain_loose_tolerance(st, a, b, W, dense, SIG_RTOL)
        assert (np.abs(got - ref) <= tol).all(), (what, got, ref, tol)
        worst[1] = max(worst[1], (np.abs(got - ref) / tol).max())
        assert (got >= 0).all() and (np.diff(got) >= 0).all(), (what, got)
    print(f"[gain] {what}: largest error / bound {worst[0]:.3f} (tight, the device's own Sigma), {worst[1]:.2e} (loose, the dense inverse)")
    return worst


@pytest.mark.parametrize("fixed", [(0,), (3, 41, 77)], ids=["node0", "three"])
def test_fixed_nodes(lib, fixed):
    arr = case_arrays(lib, "random1")
    g, p = _solved(lib, arr, 1, fixed=fixed)
    A = _A(g, p)
    _check_logdet(g, p, f"random1 with {fixed} fixed", A=A, fixed=fixed)
    f0 = fixed[0]
    bad, pre = g.logdet_sets(p, [[5, f0, 9], [12, 60], [f0]])
    assert bad == 2 and np.isfinite(pre[0][0]) and np.isnan(pre[0][1:]).all() and np.isfinite(pre[1]).all() and np.isnan(pre[2]).all()
    st = g.states()
    hyps = [_candidates(st, [f0, 7, 5], [5, f0, 7], 3), _candidates(st, [f0], [50], 4)]
    bad, gains = g.info_gain_xyt(p, hyps)
    assert bad == 0 and all(np.isfinite(x).all() for x in gains)
    _check_gain(g, p, st, hyps, gains, dense_sigma(g.l_points(), *g.arrays()[1:], p.c.tikhanov, None, fixed), f"fixed {fixed}")
    p.destroy(); g.destroy()


# ---- 6. logdet_sets --------------------------------------------------------------------------------------------------------------------------------
def _check_sets(g, p, sets, dense, what):
    """prefixes against slogdet of the device's own marginals_set (tight) and against the dense inverse (loose)"""
    bad, pre = g.logdet_sets(p, sets)
    assert bad == 0 and len(pre) == len(sets)
    worst = [0.0, 0.0]
    for s, got in zip(sets, pre):
        s = np.asarray(s, np.int32)
        M = g.marginals_set(p, s)
        tight = IM.set_tight_tolerance(M)
        ref = np.array([np.linalg.slogdet(M[:3 * j, :3 * j])[1] for j in range(1, len(s) + 1)])
        assert (np.abs(got - ref) <= tight).all(), (what, s, got, ref, tight)
        worst[0] = max(worst[0], (np.abs(got - ref) / tight).max())
        ref, loose = IM.set_prefixes(dense, s), IM.set_loose_tolerance(M, dense, s, SIG_RTOL)
        assert (np.abs(got - ref) <= loose).all(), (what, s, got, ref, loose)
        worst[1] = max(worst[1], (np.abs(got - ref) / loose).max())
    print(f"[sets] {what}: largest error / bound {worst[0]:.3f} (tight, slogdet of the device's own marginals_set), {worst[1]:.2e} (loose, the dense inverse)")
    return pre


@pytest.fixture(scope="module")
def scene(lib):
    arr = case_arrays(lib, "random2")
    g, p = _solved(lib, arr, 2)
    dense = np.linalg.inv(_A(g, p))
    yield dict(lib=lib, arr=arr, g=g, p=p, dense=dense, st=g.states())
    p.destroy(); g.destroy()


def test_sets_of_every_size_and_place(scene):
    lib, arr, g, p, dense = (scene[k] for k in ("lib", "arr", "g", "p", "dense"))
    N = len(arr[0])
    rng = np.random.default_rng(5)
    sets = [rng.choice(N, k, replace=False) for k in (1, 2, 15, 16)]
    P = PlanView(lib, N, arr[1], arr[2], xy=arr[0][:, :2])
    t = int(np.argmax(P.front_nsb))
    sets.append(P.perm[P.front_first[t]:P.front_first[t] + P.front_nsb[t]][:6])             # within one front
    leaves = np.setdiff1d(np.arange(P.nF), P.front_parent[P.front_parent >= 0])[:6]
    sets.append(P.perm[P.front_first[leaves]])                                              # one node of each of six leaves
    sets += [sets[2][::-1].copy(), np.unique(np.r_[sets[1], sets[3][:5]])]                                # nodes repeated across sets
    r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    pre = _check_sets(g, p, sets, dense, "random2, two steps")
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0
    again = g.logdet_sets(p, sets)[1]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(pre, again))
    # a set cut to its first j nodes, in the same call and in a call of its own, reproduces prefix j bit for bit
    full = sets[3]
    cuts = g.logdet_sets(p, [full] + [full[:j] for j in range(1, 16)])[1]
    for j in range(1, 16):
        assert cuts[j].tobytes() == cuts[0][:j].tobytes() == pre[3][:j].tobytes(), j
        assert g.logdet_sets(p, [full[:j]])[1][0].tobytes() == pre[3][:j].tobytes(), j


def test_two_hundred_sets_in_one_call(scene):
    g, p, dense = scene["g"], scene["p"], scene["dense"]
    rng = np.random.default_rng(9)
    pool = rng.choice(len(scene["st"]), 40, replace=False)
    sets = [rng.choice(pool, int(rng.integers(1, 17)), replace=False) for _ in range(200)]
    bad, pre = g.logdet_sets(p, sets)
    assert bad == 0
    for k in range(0, 200, 23):
        assert g.logdet_sets(p, [sets[k]])[1][0].tobytes() == pre[k].tobytes(), k
    _check_sets(g, p, sets[:6], dense, "six of 200 sets")


def test_all_nodes_of_a_16_node_graph_give_minus_logdet(lib):
    arr = datasets.random_pose_graph(16, 9, 4)
    g, p = _solved(lib, arr, 2)
    A = _A(g, p)
    nodes = np.random.default_rng(1).permutation(16)
    bad, pre = g.logdet_sets(p, [nodes])
    ld = g.logdet(p)
    M = g.marginals_set(p, nodes)
    tol = IM.logdet_tolerance(A) + IM.set_tight_tolerance(M)[-1] + IM.set_loose_tolerance(M, np.linalg.inv(A), nodes, SIG_RTOL)[-1]
    print(f"[sets] all 16 nodes: ln det Sigma {pre[0][-1]:.12g}, -logdet {-ld:.12g}, difference {abs(pre[0][-1] + ld):.2e}, bound {tol:.2e}")
    assert bad == 0 and abs(pre[0][-1] + ld) <= tol
    p.destroy(); g.destroy()


def test_sets_across_components_add_up(lib):
    arr, comp = two_components()
    g, p = _solved(lib, arr)
    n0 = np.nonzero(comp == 0)[0]; n1 = np.nonzero(comp == 1)[0]
    A, B = n0[[0, 7, 200, 399]], n1[[3, 50, 79]]
    AB = np.r_[A, B]
    bad, (lA, lB, lAB) = g.logdet_sets(p, [A, B, AB])
    tol = sum(IM.set_tight_tolerance(g.marginals_set(p, x))[-1] for x in (A, B, AB))
    print(f"[sets] across components: ln det Sigma_AuB - ln det Sigma_A - ln det Sigma_B = {lAB[-1] - lA[-1] - lB[-1]:.2e}, bound {tol:.2e}")
    assert bad == 0 and abs(lAB[-1] - lA[-1] - lB[-1]) <= tol
    p.destroy(); g.destroy()


# ---- 7. info_gain_xyt ------------------------------------------------------------------------------------------------------------------------------
def _hyps(st, seed=8):
    """hypotheses of 1, 2, 5 and 16 candidates on a pool of ten poses: shared nodes, a repeated pair, a pair the other way round"""
    rng = np.random.default_rng(seed)
    pool = rng.choice(len(st), 10, replace=False)
    ia = rng.integers(0, 10, 24)
    a = pool[ia]; b = pool[(ia + rng.integers(1, 10, 24)) % 10]
    a[5], b[5] = a[3], b[3]                                      # (3..7 is the m = 5 hypothesis) the pair of 3 again
    a[7], b[7] = b[4], a[4]                                      # the pair of 4 the other way round
    cand = _candidates(st, a, b, seed + 1)
    return [tuple(x[k] for x in cand) for k in (slice(0, 1), slice(1, 3), slice(3, 8), slice(8, 24))]


def test_gain_matches_the_model_and_the_gate(scene):
    g, p, st, dense = scene["g"], scene["p"], scene["st"], scene["dense"]
    hyps = _hyps(st)
    assert [len(h[0]) for h in hyps] == [1, 2, 5, 16]
    r0 = scene["lib"].dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    bad, gains = g.info_gain_xyt(p, hyps)
    assert bad == 0 and scene["lib"].dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0
    _check_gain(g, p, st, hyps, gains, dense, "random2, two steps")
    again = g.info_gain_xyt(p, hyps)[1]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(gains, again))
    cuts = g.info_gain_xyt(p, [tuple(x[:j] for x in hyps[3]) for j in range(1, 16)])[1]
    for j in range(1, 16):
        assert cuts[j - 1].tobytes() == gains[3][:j].tobytes(), j
    # the C that gate_xyt_joint returns for the same hypotheses, with any z
    rng = np.random.default_rng(3)
    gate = [(a, b, np.array([predict(st[i], st[j]) for i, j in zip(a, b)]) + rng.normal(size=(len(a), 3)), W) for a, b, W in hyps]
    _, _, Cs = g.gate_xyt_joint(p, gate)
    worst = 0.0
    for (a, b, W), Cm, got in zip(hyps, Cs, gains):
        lw = sum(np.linalg.slogdet(w.reshape(3, 3))[1] for w in W)
        ref = 0.5 * (np.linalg.slogdet(Cm)[1] + lw)
        tol = IM.gain_tight_tolerance(st, a, b, W, _device_sigma(g, p, np.r_[a, b]))[-1]
        assert abs(got[-1] - ref) <= tol, (got[-1], ref, tol)
        worst = max(worst, abs(got[-1] - ref) / tol)
    print(f"[gain] against slogdet of gate_xyt_joint's C: largest error / bound {worst:.3f}")


def test_gain_is_what_logdet_grows_by_when_the_factors_are_added(lib):
    arr = case_arrays(lib, "random1")
    g, p = _solved(lib, arr, 0)
    for it in range(60):
        g.cholesky(p)
        if np.abs(g.deltas()).max() < 1e-13:
            break
    assert np.abs(g.deltas()).max() < 1e-13, np.abs(g.deltas()).max()
    g.cholesky(p)                                                # (the factor of the system AT the converged states)
    st = g.states()
    assert np.abs(st - g.l_points()).max() < 1e-12
    before, _, tol0 = _check_logdet(g, p, "random1, converged")
    a, b, W = _candidates(st, [3, 70, 12, 3], [55, 12, 70, 20], 6)
    bad, gains = g.info_gain_xyt(p, [(a, b, W)])
    assert bad == 0
    for i in range(4):
        g.add_factor_xyt(int(a[i]), int(b[i]), predict(st[a[i]], st[b[i]]), W[i].reshape(3, 3))
    g.cholesky(p)
    assert np.abs(g.l_points() - st).max() < 1e-12
    after, _, tol1 = _check_logdet(g, p, "random1, four factors added")
    print(f"[gain] end to end: 2 gain {2 * gains[0][-1]:.12g}, logdet grew by {after - before:.12g}, difference {abs(2 * gains[0][-1] - (after - before)):.2e}, "
          f"bound {tol0 + tol1:.2e}")
    assert abs(2 * gains[0][-1] - (after - before)) <= tol0 + tol1
    p.destroy(); g.destroy()


# ---- 8. non-interference and refusals ------------------------------------------------------------------------------------------------------------
def test_the_calls_leave_every_other_output_bitwise_unchanged(lib):
    arr = datasets.random_pose_graph(400, 350, 2)
    runs = []
    for with_calls in (False, True):
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        snaps = []
        for it in range(3):
            g.cholesky(p)
            if with_calls:
                r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
                g.logdet(p); g.logdet_sets(p, [[5, 399, 17], [3]]); g.info_gain_xyt(p, [_candidates(g.states(), [3, 100, 399], [250, 3, 7], it)])
                assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0
            d2, S = g.gate_xyt(p, [3, 9], [200, 4], np.zeros((2, 3)), np.tile(np.diag([100.0, 100.0, 400.0]).ravel(), (2, 1)))
            X = g.solve(p, np.arange(3.0 * 400).reshape(1, -1))
            snaps.append(b"".join(np.ascontiguousarray(x).tobytes() for x in (g.states(), g.deltas(), g.l_points(), g.marginals(p), d2, S, X)))
        runs.append(snaps)
        p.destroy(); g.destroy()
    assert runs[0] == runs[1]


def _raw(lib, g, p):
    """the three calls on sentinel-filled outputs: (codes, nothing written and every code recorded)"""
    ptr = np.array([0, 2, 3], np.int32); nodes = np.array([4, 9, 1], np.int32); b = np.array([7, 4, 30], np.int32)
    W = np.tile(np.diag([100.0, 100.0, 400.0]).ravel(), (3, 1))
    o1, o2, o3 = np.full(2, SENT), np.full(5, SENT), np.full(5, SENT)
    d, clean, codes = lib.dll, True, []
    for call, out in ((lambda: d.aprilsam_amd_logdet(g.ptr, p.ptr, o1.ctypes.data_as(_dp)), o1),
                      (lambda: d.aprilsam_amd_logdet_sets(g.ptr, p.ptr, 2, ptr.ctypes.data_as(_ip), nodes.ctypes.data_as(_ip), o2.ctypes.data_as(_dp)), o2),
                      (lambda: d.aprilsam_amd_info_gain_xyt(g.ptr, p.ptr, 2, ptr.ctypes.data_as(_ip), nodes.ctypes.data_as(_ip), b.ctypes.data_as(_ip),
                                                            W.ctypes.data_as(_dp), o3.ctypes.data_as(_dp)), o3)):
        lib.clear_error()
        codes.append(call())
        if codes[-1] < 0:
            clean = clean and bool(np.all(out == SENT)) and lib.last_error()[0] == codes[-1]
    return codes, clean


def test_refusals_write_nothing_and_leave_the_factor(lib):
    from tests.test_gpu_consumer_refusals import _asymmetric_scene, _shard
    ctx = rc.Ctx(lib)
    g, p = ctx.g, ctx.p
    assert _raw(lib, g, p) == ([-1, -1, -1], True)                                          # before any solve
    ctx.start()
    assert _raw(lib, g, p) == ([0, 0, 0], True)
    ref = g.logdet(p), g.logdet_sets(p, [[4, 9, 1]])[1][0].tobytes()
    N = g.n_nodes
    for bad_node in (N, -1):                                                                # out of range
        nodes = np.array([4, bad_node], np.int32); ptr = np.array([0, 2], np.int32); out = np.full(3, SENT); W = np.diag([1.0, 1.0, 1.0]).ravel()
        assert lib.dll.aprilsam_amd_logdet_sets(g.ptr, p.ptr, 1, ptr.ctypes.data_as(_ip), nodes.ctypes.data_as(_ip), out.ctypes.data_as(_dp)) == -13
        one = np.array([0, 1], np.int32); a = np.array([4], np.int32); b = np.array([bad_node], np.int32)
        assert lib.dll.aprilsam_amd_info_gain_xyt(g.ptr, p.ptr, 1, one.ctypes.data_as(_ip), a.ctypes.data_as(_ip), b.ctypes.data_as(_ip), W.ctypes.data_as(_dp),
                                                  out.ctypes.data_as(_dp)) == -13
        assert np.all(out == SENT)
    assert g.logdet_sets(p, []) == (0, []) and g.info_gain_xyt(p, []) == (0, [])           # n == 0
    assert (g.logdet(p), g.logdet_sets(p, [[4, 9, 1]])[1][0].tobytes()) == ref              # the factor is where it was
    rc.ev_resident_open(ctx)                                                                # a resident run in progress
    assert _raw(lib, g, p) == ([-1, -1, -1], True)
    ctx.cleanup.pop()()
    ctx.call()
    assert _raw(lib, g, p) == ([0, 0, 0], True)
    rc.ev_own_call_fails(ctx)                                                               # a step that was not positive definite
    assert _raw(lib, g, p) == ([-1, -1, -1], True)
    ctx.cleanup.pop()()
    ctx.call()
    assert _raw(lib, g, p) == ([0, 0, 0], True)
    g.optimize_lm(p, max_iters=2)                                                           # LM drops the factor
    assert _raw(lib, g, p) == ([-1, -1, -1], True)
    with pytest.raises(MarginalsError) as e:
        g.logdet(p)
    assert e.value.code == -1
    ctx.destroy()
    ctx = rc.Ctx(lib)                                                                       # a sharded param
    _shard(ctx)
    assert _raw(lib, ctx.g, ctx.p) == ([-12, -12, -12], True)
    ctx.cleanup.pop()()
    ctx.destroy()
    ctx = rc.Ctx(lib, sc=_asymmetric_scene())                                               # a factorisation of an asymmetric W
    ctx.start()
    assert _raw(lib, ctx.g, ctx.p) == ([-12, -12, -12], True)
    ctx.destroy()
