"""Comparison of the covariance entry points (aprilsam_amd_marginals / _joint / _joint_any) with numpy's inverse of the system the
step factorised, and the checkpoint selector of the M3500 incremental demo -- shared by tests/test_gpu_marginals.py,
tests/test_gpu_gating.py and tests/test_gpu_consumer_paths.py.  TEST-ONLY.  tests/test_sigma_compare.py shows on the CPU that the
comparison fails for a block off by 1e-7 of its scale, for lambda on the wrong node set and for a transposed joint block.

The error of a block is |GPU - reference| / (largest |entry| of the pose's block row of Sigma; for a pair the larger of the two).
Calibration on the CPU, two independent references of the same system: the dense inverse and scipy splu solves disagree by up to
7e-12 (M3500) and 2.2e-11 (lattice K = 60); splu with two orderings (COLAMD, MMD on A + A') by 7e-11 (K = 60) and 3.4e-10 (K = 120) --
the figure grows with the lattice's condition number.  On the graphs of tests/test_gpu_consumer_paths.py the dense inverse and splu
(COLAMD, MMD) disagree by at most 3.1e-12 (random 700 / 600 / 21), 2.9e-12 (random 3000 / 1800 / 102) and 8.4e-13 (the
two-component graph): 1e-9 keeps 300 x and more."""
import numpy as np

from tests.support.marginal_cases import factor_pairs
from tests.support.normal_eq import normal_equation_residual
from tests.support.selinv_model import dense_system, system_blocks

SIG_RTOL = 1e-9          # against the dense inverse (every graph up to 10 800 unknowns)


def ref_blocks(Sig, N, fa, fb):
    """diagonal blocks [N,3,3] and the factor pairs' joint blocks [P,6,6] of a dense Sigma"""
    a, b = factor_pairs(fa, fb)
    diag = np.stack([Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(N)])
    joint = np.stack([Sig[np.ix_(np.r_[3 * x:3 * x + 3, 3 * y:3 * y + 3], np.r_[3 * x:3 * x + 3, 3 * y:3 * y + 3])] for x, y in zip(a, b)]) \
        if len(a) else np.zeros((0, 6, 6))
    return diag, joint


def ref_joint(Sig, a, b):
    return np.stack([Sig[np.ix_(np.r_[3 * x:3 * x + 3, 3 * y:3 * y + 3], np.r_[3 * x:3 * x + 3, 3 * y:3 * y + 3])] for x, y in zip(a, b)])


def row_scale(Sig):
    N = len(Sig) // 3
    return np.abs(Sig).reshape(N, 3, 3 * N).max(axis=(1, 2))


def dense(g, p, lam_nodes=None):
    """Sigma = inv(A(l_point)) of the graph's system, lambda on the nodes [0, lam_nodes) (default: all), and its row scales"""
    states, fa, fb, z, W = g.arrays()
    Aii, Aab = system_blocks(g.l_points(), fa, fb, z, W, p.c.tikhanov, lam_nodes)
    Sig = np.linalg.inv(dense_system(Aii, Aab, fa, fb))
    return Sig, row_scale(Sig)


def check_blocks(ref, fa, fb, d, j):
    """diagonal blocks d of all poses and joint blocks j of the factor pairs against ref = (Sig, scale); returns the worst error"""
    Sig, scale = ref
    N = len(scale)
    rd, rj = ref_blocks(Sig, N, fa, fb)
    worst = (np.abs(d - rd).reshape(N, 9).max(axis=1) / scale).max()
    a, b = factor_pairs(fa, fb)
    if len(a):
        assert not np.isnan(j).any()
        ej = np.abs(j - rj).reshape(len(a), 36).max(axis=1) / np.maximum(scale[a], scale[b])
        worst = max(worst, ej.max())
    assert worst < SIG_RTOL, worst
    return worst


def check_any(ref, a, b, J):
    """joint blocks J of the pairs (a, b) against ref = (Sig, scale); returns the worst error"""
    Sig, scale = ref
    assert np.isfinite(J).all()
    err = np.abs(J - ref_joint(Sig, a, b)).reshape(len(a), 36).max(axis=1) / np.maximum(scale[a], scale[b])
    assert err.max() < SIG_RTOL, err.max()
    return err.max()


def compare_dense(g, p, lam_nodes=None, ref=None):
    """marginals of all poses and marginals_joint of every factor pair against the dense inverse; ref: a (Sig, scale) computed
    before.  Returns the worst error"""
    states, fa, fb, z, W = g.arrays()
    a, b = factor_pairs(fa, fb)
    return check_blocks(dense(g, p, lam_nodes) if ref is None else ref, fa, fb, g.marginals(p), g.marginals_joint(p, a, b) if len(a) else None)


def compare_dense_any(g, p, a, b, lam_nodes=None, ref=None):
    """marginals_joint_any of the pairs (a, b) against the dense inverse; returns the blocks"""
    J = g.marginals_joint_any(p, a, b)
    check_any(dense(g, p, lam_nodes) if ref is None else ref, a, b, J)
    return J


def random_pairs(N, seed, k=100):
    """k random pairs, the same pairs in the other order, and ten with a == b"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N, k).astype(np.int32); b = rng.integers(0, N, k).astype(np.int32)
    return np.r_[a, b, a[:10]], np.r_[b, a, a[:10]]


class Recorder:
    """lib stand-in for harness.run_demo that keeps the graph it makes"""
    def __init__(self, lib):
        self.lib, self.graphs = lib, []

    def __getattr__(self, k):
        return getattr(self.lib, k)

    def new_graph(self):
        g = self.lib.new_graph(); self.graphs.append(g)
        return g


def demo_checkpoints(rec, arr, check, batch_residual=False):
    """on_step for harness.run_demo(rec, arr, ...): calls check(g, p, k, lam_nodes) after every batch step (first pose, fall-backs),
    every re-planned step, the first five steps that took low-rank updates of their root path, the first twelve loop closures on
    the fast path and every 50th step.  lam_nodes: None after a batch step, else the number of poses of the last batch step.
    Returns (on_step, seen); seen counts the checkpoints of each kind"""
    seen = dict(batch=0, replanned=0, updated=0, fast=0, n_batch=0)
    closes = {max(int(a), int(b)) for a, b in zip(arr[1], arr[2]) if b >= 0 and abs(int(a) - int(b)) > 1}

    def on_step(k, p, was_batch):
        g = rec.graphs[-1]
        st = p.stats()
        if was_batch:
            seen["n_batch"] = k + 1
            if batch_residual:
                out = normal_equation_residual(g.l_points(), *g.arrays()[1:], g.deltas(), p.c.tikhanov)
                assert out["rel_max"] < 1e-10, out
        kind = "batch" if was_batch else "replanned" if st["inc_replanned"] == 1 else "updated" if st["inc_fronts_updated"] > 0 else "fast"
        if kind in ("batch", "replanned") or (kind == "updated" and seen["updated"] < 5) or \
                (kind == "fast" and (k % 50 == 0 or (k in closes and seen["fast"] < 12))):
            check(g, p, k, None if was_batch else seen["n_batch"])
            seen[kind] += 1
    return on_step, seen
