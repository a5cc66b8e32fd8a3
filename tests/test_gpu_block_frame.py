"""The edges of the frame under aprilsam_amd_gate_xyt_joint, aprilsam_amd_info_gain_xyt and aprilsam_amd_logdet_sets (k_block_chol,
aprilsam_amd/csrc/jointgate.hip.h): list lengths around the trips of its 64-thread stride over the lower blocks --
m = 10 (55 blocks, one trip), m = 11 (66, the first length with a second trip), m = 16 (136, a third) and m = 1 -- in ONE call to each
entry point, the three riders held to each other through the matrix the joint gate returns, the bitwise prefix property between the
lengths, and a pivot that is not positive behind the first trip.  What the other lengths, places and refusals owe: test_gpu_joint_gate.py,
test_gpu_info.py.

The lists are nested (each the first m entries of the longest), so every shorter list is a truncation of every longer one.  Bounds: the
project's GATE_RTOL, relative to the value."""
import numpy as np
import pytest

from tests.support.gate_model import predict
from tests.test_gpu_gating import GATE_RTOL
from tests.test_joint_gate_model import chain_scenario

pytestmark = pytest.mark.gpu
LENGTHS = [1, 10, 11, 16]
FIXED = 17


@pytest.fixture(scope="module")
def scene(lib):
    """the 30-pose open chain after one step with one node fixed; 16 candidates on a pool of ten free poses (shared nodes, a repeated pair, a pair both
    ways round), 16 free nodes for the sets"""
    arr = chain_scenario()[0]
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    assert g.set_fixed(FIXED) == 0
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    st = g.states()
    rng = np.random.default_rng(33)
    free = np.setdiff1d(np.arange(len(st)), [FIXED])
    nodes = rng.choice(free, 16, replace=False).astype(np.int32)
    pool = nodes[:10]
    ia = rng.integers(0, 10, 16)
    a = pool[ia]; b = pool[(ia + rng.integers(1, 10, 16)) % 10]
    a[4], b[4] = a[2], b[2]                                      # the pair of 2 again
    a[12], b[12] = b[3], a[3]                                    # the pair of 3 the other way round, behind the first trip
    z = np.array([predict(st[i], st[j]) for i, j in zip(a, b)]) + rng.normal(size=(16, 3)) * 0.3
    L = rng.normal(size=(16, 3, 3)) * 0.3 + np.eye(3) * 3
    W = np.einsum("nij,nkj->nik", L, L).reshape(16, 9)
    a, b = a.astype(np.int32), b.astype(np.int32)
    gate = [(a[:m], b[:m], z[:m], W[:m]) for m in LENGTHS]
    gain = [(a[:m], b[:m], W[:m]) for m in LENGTHS]
    sets = [nodes[:m] for m in LENGTHS]
    yield dict(g=g, p=p, W=W, nodes=nodes, gate=gate, gain=gain, sets=sets,
               out=(g.gate_xyt_joint(p, gate), g.info_gain_xyt(p, gain), g.logdet_sets(p, sets)))
    p.destroy(); g.destroy()


def _close(got, ref, what):
    err = np.abs(got - ref) / np.abs(ref)
    print(f"[frame] {what}: largest relative error {err.max():.2e} (bound {GATE_RTOL:.0e})")
    assert np.isfinite(got).all() and (err <= GATE_RTOL).all(), (what, got, ref)


def test_gain_is_half_the_logdet_of_the_gates_own_matrix(scene):
    (bad_d, d2, Cs), (bad_g, gains), _ = scene["out"]
    assert bad_d == 0 and bad_g == 0 and [len(x) for x in gains] == LENGTHS == [len(x) for x in d2]
    lw = np.cumsum([np.linalg.slogdet(w.reshape(3, 3))[1] for w in scene["W"]])
    for m, Cm, got in zip(LENGTHS, Cs, gains):
        assert Cm.shape == (3 * m, 3 * m) and np.array_equal(Cm, Cm.T)
        ref = np.array([0.5 * (np.linalg.slogdet(Cm[:3 * j + 3, :3 * j + 3])[1] + lw[j]) for j in range(m)])
        _close(got, ref, f"gain, m = {m}")


def test_set_prefixes_are_slogdet_of_marginals_set(scene):
    g, p = scene["g"], scene["p"]
    bad, pre = scene["out"][2]
    assert bad == 0 and [len(x) for x in pre] == LENGTHS
    M = g.marginals_set(p, scene["nodes"])
    for m, got in zip(LENGTHS, pre):
        ref = np.array([np.linalg.slogdet(M[:3 * j + 3, :3 * j + 3])[1] for j in range(m)])
        _close(got, ref, f"sets, m = {m}")


def test_shorter_lists_are_bitwise_the_prefixes_and_two_calls_agree(scene):
    g, p = scene["g"], scene["p"]
    (_, d2, Cs), (_, gains), (_, pre) = scene["out"]
    for k, m in enumerate(LENGTHS[:-1]):
        for longer in (2, 3):                                   # against the m = 11 and the m = 16 list
            if longer <= k:
                continue
            for out in (d2, gains, pre):
                assert out[k].tobytes() == out[longer][:m].tobytes(), (m, LENGTHS[longer])
            assert Cs[k].tobytes() == np.ascontiguousarray(Cs[longer][:3 * m, :3 * m]).tobytes(), (m, LENGTHS[longer])
    (_, d2b, Csb), (_, gainsb), (_, preb) = g.gate_xyt_joint(p, scene["gate"]), g.info_gain_xyt(p, scene["gain"]), g.logdet_sets(p, scene["sets"])
    for x, y in zip(d2 + Cs + gains + pre, d2b + Csb + gainsb + preb):
        assert x.tobytes() == y.tobytes()


def test_a_zero_pivot_behind_the_first_trip_ends_the_prefixes_there(scene):
    """a fixed node's rows are exact zeros: as entry 10 of a set of 13 its pivot is column 30, formed by blocks of the second trip"""
    g, p, nodes = scene["g"], scene["p"], scene["nodes"]
    bad, pre = g.logdet_sets(p, [np.r_[nodes[:10], FIXED, nodes[10:12]].astype(np.int32), nodes[:10]])
    assert bad == 1
    assert np.isfinite(pre[0][:10]).all() and np.isnan(pre[0][10:]).all() and len(pre[0]) == 13
    assert pre[0][:10].tobytes() == pre[1].tobytes() == scene["out"][2][1][1].tobytes()
