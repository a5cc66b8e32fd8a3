"""The consumers of the retained factor (aprilsam_amd_marginals, _marginals_joint, _marginals_joint_any) behind every launch form of
an incremental step: the extended structure differs from form to form -- tail fronts in padded layout (inc_tail, tail_poses),
regenerated fronts at new offsets (inc_one, inc_multi), low-rank-updated fronts (inc_update, inside k_inc_one with inc_one_up / _dn)
-- and selinv.hip.h and pathsolve.hip.h rebuild their tables from it.  The M3500 demo under each form at the checkpoints of
tests/test_gpu_marginals.py, and four growth scenarios of tests/test_gpu_inc_exact.py after every step.

Sigma = inv(A(l_point)) with lambda on the poses present at the last batch step, compared at SIG_RTOL = 1e-9
of the block row's largest entry (tests/support/sigma_compare.py; two CPU references of Sigma disagree by at most 7e-12 on M3500)."""
import numpy as np
import pytest

from aprilsam_amd import datasets, harness
from tests.support.sigma_compare import Recorder, compare_dense, compare_dense_any, demo_checkpoints, dense, random_pairs
from tests.test_gpu_inc_exact import GROWTH

pytestmark = pytest.mark.gpu
FORMS = [{"inc_tail": 0}, {"inc_tail": 0, "inc_one": 0}, {"inc_multi": 0}, {"tail_poses": 8}, {"inc_update": 0},
         {"inc_update": 1, "inc_one_up": 16, "inc_one_dn": 16}, {"inc_one_threads": 1024}, {"inc_lazy_states": 0}, {"inc_tail_solve": 0},
         {"pool_poison": 1}]


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _check(g, p, seed, lam_nodes, k_pairs):
    """diagonal blocks, factor-pair blocks and joint_any of k_pairs random pairs (both orders, and a == b) against one dense inverse"""
    ref = dense(g, p, lam_nodes)
    worst = compare_dense(g, p, ref=ref)
    a, b = random_pairs(g.n_nodes, seed, k_pairs)
    compare_dense_any(g, p, a.astype(np.int32), b.astype(np.int32), ref=ref)
    return worst


@pytest.mark.parametrize("opts", FORMS, ids=_ids)
def test_demo_checkpoints_under_every_launch_form(lib, opts):
    """first 600 steps of the M3500 demo: every batch, re-planned and fall-back step, the first low-rank-updated steps, the first loop
    closures on the fast path and every 50th step; the run's chi^2 trace and states bitwise those of the same-options run without
    any consumer call"""
    arr = datasets.m3500_arrays()
    worst = [0.0]
    with lib.options(**opts):
        plain = harness.run_demo(lib, arr, max_poses=600, record_states_every=50)
        rec = Recorder(lib)

        def check(g, p, k, lam_nodes):
            worst[0] = max(worst[0], _check(g, p, k, lam_nodes, 60))
        on_step, seen = demo_checkpoints(rec, arr, check, batch_residual=True)
        res = harness.run_demo(rec, arr, max_poses=600, record_states_every=50, on_step=on_step)
    print(f"[consumers-inc] {_ids(opts)}: checkpoints {seen}, worst {worst[0]:.2e}")
    assert seen["batch"] >= 5 and seen["fast"] >= 12, seen
    if opts.get("inc_update", 1) == 0 or opts.get("inc_multi", 1) == 0:        # (low-rank updates ride on the multi-level launch)
        assert seen["updated"] == 0, seen
    else:
        assert seen["updated"] >= 1, seen
    assert res["chi2"].tobytes() == plain["chi2"].tobytes()
    assert res["final_states"].tobytes() == plain["final_states"].tobytes()
    for k in plain["snaps"]:
        assert res["snaps"][k].tobytes() == plain["snaps"][k].tobytes()


class _ConsumerGraph:
    """a graph whose every solver call is followed by the consumers, checked against the dense inverse"""
    def __init__(self, owner, g):
        self.owner, self.g = owner, g
        self.n_batch = 0

    def __getattr__(self, k):
        return getattr(self.g, k)

    def cholesky(self, p):
        self.g.cholesky(p)
        self.n_batch = self.g.n_nodes
        self._after(p, None)

    def cholesky_inc(self, p):
        bt = p.c.batch_time
        self.g.cholesky_inc(p)
        if p.c.batch_time != bt:                          # a fall-back batch rewrites batch_time
            self.n_batch = self.g.n_nodes
            self.owner.fallbacks += 1
            self._after(p, None)
        else:
            self.owner.replanned += p.stats()["inc_replanned"] == 1
            self._after(p, self.n_batch)

    def _after(self, p, lam_nodes):
        o = self.owner
        o.steps += 1
        o.worst = max(o.worst, _check(self.g, p, o.steps, lam_nodes, 40))


class _ConsumerLib:
    """lib stand-in for the growth drivers"""
    def __init__(self, lib):
        self.lib = lib
        self.steps = self.fallbacks = self.replanned = 0
        self.worst = 0.0

    def __getattr__(self, k):
        return getattr(self.lib, k)

    def new_graph(self):
        return _ConsumerGraph(self, self.lib.new_graph())


@pytest.mark.parametrize("name", ["random_growth_old_old_30", "recent_growth_12", "late_priors", "tutorial"])
def test_growth_scenarios_after_every_step(lib, name):
    """cross-branch re-plans, growth among the newest poses with short tail fronts, priors arriving late, the tutorial: marginals,
    factor-pair blocks and joint_any after every step (at most 150 poses)"""
    L = _ConsumerLib(lib)
    GROWTH[name](L)
    print(f"[consumers-inc] {name}: {L.steps} steps, {L.fallbacks} fall-backs, {L.replanned} re-planned, worst {L.worst:.2e}")
    assert L.steps >= (6 if name == "tutorial" else 60)
    if name == "random_growth_old_old_30":
        assert L.replanned > 0 and L.fallbacks > 0
