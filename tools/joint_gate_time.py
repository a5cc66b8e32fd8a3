#!/usr/bin/env python3
"""Time aprilsam_amd_gate_xyt_joint (joint compatibility gating) on M3500 and the 10^5-pose lattice, with
aprilsam_amd_gate_xyt on the same candidates, gated one by one, as the yardstick; and count, on the held-out M3500 scenario of
tests/test_pathsolve_model.py (m3500_gate_scenario), how many of the 100 false candidates the joint test rejects.

    python tools/joint_gate_time.py [--cases m3500,lattice316] [--hyps 1,100,1000] [--sizes 4,16] [--reps 5]

Hypotheses: a front end's branch-and-bound level around the newest pose.  The candidate pool joins each of the last 8 poses to each of
the 32 older poses nearest (in x, y) to the newest one; a hypothesis is m distinct candidates of the pool, so the hypotheses of one call
share their 40 nodes and at most 780 node pairs, each solved once per call.  One JSON line per (case, hypotheses, m): ms of the first call
after a solve (it also builds the host table of the factor's fronts), the median of the repeat calls, the median for gate_xyt on the
n_hyp m candidates, the distinct nodes and node pairs of the call.

The scenario line: M3500 solved without its last 100 loop closures; every false candidate (a true closure's z, W on a wrong pair of
poses) is sent as the last of a 3-candidate hypothesis behind the two held-out true closures nearest (x, y distance of an end pose, at
the solved states) to its two poses.  Counted at the 0.999 quantiles: rejected alone (gate_xyt, 3 dof), by the whole hypothesis (9 dof), by
its conditional distance d2_prefix[2] - d2_prefix[1] (3 dof); and the true pairs in front that pass their own joint test (6 dof)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gate_time import arrays_for  # noqa: E402


def pool_of(states, last=8, near=32):
    """candidate pool (a, b): each of the last `last` poses against the `near` older poses nearest to the newest one"""
    N = len(states)
    older = np.arange(N - last)
    d = np.hypot(*(states[older, :2] - states[N - 1, :2]).T)
    nb = older[np.argsort(d, kind="stable")[:near]]
    a = np.repeat(np.arange(N - last, N), len(nb)); b = np.tile(nb, last)
    return a.astype(np.int32), b.astype(np.int32)


def hypotheses(states, n_hyp, m, seed=0):
    from tests.support.gate_model import predict
    rng = np.random.default_rng(seed)
    pa, pb = pool_of(states)
    W = np.tile(np.diag([100.0, 100.0, 1000.0]).ravel(), (m, 1))
    out = []
    for _ in range(n_hyp):
        k = rng.choice(len(pa), m, replace=False)
        z = np.array([predict(states[i], states[j]) for i, j in zip(pa[k], pb[k])]) + rng.normal(size=(m, 3)) * 0.05
        out.append((pa[k], pb[k], z, W))
    return out


def raw_joint(lib, g, p, hyps, flat):
    """the C call on arrays laid out beforehand (host.Graph.gate_xyt_joint concatenates its list of hypotheses on every call)"""
    from aprilsam_amd.host import _np_d, _np_i
    ms = [len(h[0]) for h in hyps]
    ptr = np.concatenate([[0], np.cumsum(ms)]).astype(np.int32)
    a, b, z, W = (np.ascontiguousarray(x) for x in flat)
    d2 = np.empty(len(a)); Cm = np.empty(sum(9 * m * m for m in ms))

    def call():
        rc = lib.dll.aprilsam_amd_gate_xyt_joint(g.ptr, p.ptr, len(hyps), _np_i(ptr), _np_i(a), _np_i(b), _np_d(z), _np_d(W), _np_d(d2), _np_d(Cm))
        assert rc == 0, (rc, lib.last_error())
    return call


def timed(f, reps):
    t0 = time.perf_counter(); f(); first = (time.perf_counter() - t0) * 1e3
    rep = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); rep.append((time.perf_counter() - t0) * 1e3)
    return round(first, 3), round(float(np.median(rep)), 3)


def scenario(lib):
    from scipy.stats import chi2
    from tests.test_pathsolve_model import GATE_ITERS, m3500_gate_scenario
    ho, a, b, z, W = m3500_gate_scenario(None)
    g = lib.new_graph(); g.build_from_arrays(*ho); p = lib.new_param()
    for _ in range(GATE_ITERS):
        g.cholesky(p)
    xy = g.states()[:, :2]
    single, _ = g.gate_xyt(p, a, b, z, W)
    hyps = []
    for f in range(100, 200):
        front = []
        for q in (a[f], b[f]):
            d = np.minimum(np.hypot(*(xy[a[:100]] - xy[q]).T), np.hypot(*(xy[b[:100]] - xy[q]).T))
            front.append(next(int(t) for t in np.argsort(d, kind="stable") if int(t) not in front))
        k = np.array(front + [f])
        hyps.append((a[k], b[k], z[k], W[k]))
    t0 = time.perf_counter(); bad, d2, _ = g.gate_xyt_joint(p, hyps); ms = (time.perf_counter() - t0) * 1e3
    d2 = np.array(d2)
    q3, q6, q9 = (chi2.ppf(0.999, k) for k in (3, 6, 9))
    out = dict(scenario="m3500 without its last 100 closures", false_candidates=100, not_positive=int(bad),
               rejected_alone=int((single[100:] > q3).sum()), rejected_by_whole_hypothesis=int((d2[:, 2] > q9).sum()),
               rejected_by_conditional_distance=int((d2[:, 2] - d2[:, 1] > q3).sum()), true_pairs_in_front_accepted=int((d2[:, 1] < q6).sum()),
               ms_call=round(ms, 3))
    p.destroy(); g.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice316")
    ap.add_argument("--hyps", default="1,100,1000")
    ap.add_argument("--sizes", default="4,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-scenario", action="store_true")
    o = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import host
    lib = host.SolverLib()
    for name in [c for c in o.cases.split(",") if c]:
        arr = arrays_for(lib, name)
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        g.cholesky(p)
        t0 = time.perf_counter(); g.cholesky(p); step_ms = (time.perf_counter() - t0) * 1e3
        st = g.states()
        for n_hyp in [int(x) for x in o.hyps.split(",")]:
            for m in [int(x) for x in o.sizes.split(",")]:
                hyps = hypotheses(st, n_hyp, m)
                flat = tuple(np.concatenate([h[k] for h in hyps]) for k in range(4))
                nodes = np.unique(np.r_[flat[0], flat[1]])
                pairs = set()
                for h in hyps:
                    q = np.unique(np.r_[h[0], h[1]])
                    pairs.update((int(x), int(y)) for i, x in enumerate(q) for y in q[i + 1:])
                g.cholesky(p)                                   # a new factor: the first call builds the front table again
                jf, jm = timed(raw_joint(lib, g, p, hyps, flat), o.reps)
                _, sm = timed(lambda: g.gate_xyt(p, *flat), o.reps)
                print(json.dumps(dict(case=name, poses=len(st), hypotheses=n_hyp, candidates_each=m, distinct_nodes=len(nodes), distinct_pairs=len(pairs),
                                      ms_gate_xyt_joint_first=jf, ms_gate_xyt_joint=jm, ms_gate_xyt_same_candidates=sm,
                                      ms_solver_step=round(step_ms, 3))), flush=True)
        p.destroy(); g.destroy()
    if not o.no_scenario:
        print(json.dumps(scenario(lib)), flush=True)


if __name__ == "__main__":
    main()
