#!/usr/bin/env python3
"""Time aprilsam_amd_marginal_prior and aprilsam_amd_graph_marginalize on M3500, and what one 11-node dense Gaussian factor costs a
resident step.

    python tools/marginal_prior_time.py [--reps 7] [--rounds 6] [--steps 200] [--out profiles/marginal_prior.txt]

One JSON line per measurement, wall clock of the Python call in ms:
  prior       after one april_graph_cholesky, the prior of the oldest 1, 8 and 24 poses: the first call, the median of --reps repeats, and
              -- the yardstick, in the same run -- numpy's dense Schur complement of the same blocks on the host (model of tests/support/,
              float64, the system assembled beforehand: the solve and the products alone).  A set the call refuses is recorded with its code.
  marginalize aprilsam_amd_graph_marginalize of the oldest 8 poses (4, 2, 1 when the blanket is too large for a factor), then the next
              (cold: new plan) april_graph_cholesky
  resident    ms per resident step (aprilsam_amd_batch_resident, --steps steps, the median of the steps) of M3500 as it is and of M3500
              carrying one Gaussian factor on 11 nodes -- consecutive poses, and poses 37 apart -- alternating, --rounds times each (the
              order of a round alternates too)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginal_prior.txt"))
    o = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import datasets, host
    from tests.support import marginal_prior_model as mm
    lib = host.SolverLib()
    arr = datasets.m3500_batch()
    st, fa, fb, z, W = arr
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw)); print(lines[-1], flush=True)

    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.cholesky(p)
    lp = g.l_points()
    for m in (1, 8, 24):
        remove = list(range(m))
        try:
            first, got = timed(lambda: g.marginal_prior(p, remove))
        except RuntimeError as e:
            FM, B = mm.blanket(fa, fb, remove)
            emit(what="prior", removed=m, blanket=len(B), refused=int(e.args[0]))
            continue
        rep = [timed(lambda: g.marginal_prior(p, remove))[0] for _ in range(o.reps)]
        FM, B = mm.blanket(fa, fb, remove)
        sub = sorted(set(remove) | set(B)); loc = {n: i for i, n in enumerate(sub)}
        H, gg = mm.dense_system(lp[sub], [loc[int(a)] for a in fa[FM]], [loc[int(b)] if b >= 0 else -1 for b in fb[FM]], z[FM], np.asarray(W).reshape(-1, 3, 3)[FM])
        rows_m, rows_b = mm._rows([loc[i] for i in remove]), mm._rows([loc[i] for i in B])

        def schur():
            X = np.linalg.solve(H[np.ix_(rows_m, rows_m)], np.column_stack([H[np.ix_(rows_m, rows_b)], gg[rows_m]]))
            return H[np.ix_(rows_b, rows_b)] - H[np.ix_(rows_b, rows_m)] @ X[:, :-1], gg[rows_b] - H[np.ix_(rows_b, rows_m)] @ X[:, -1]
        host_ms = [timed(schur)[0] for _ in range(o.reps)]
        L, _ = schur()
        emit(what="prior", removed=m, blanket=len(B), entries=len(FM), ms_first=round(first, 3), ms_repeat=round(float(np.median(rep)), 3),
             ms_repeat_all=[round(x, 3) for x in rep], ms_numpy_schur=round(float(np.median(host_ms)), 3),
             max_abs_diff_lambda=float(np.max(np.abs(L - got[3]))), reps=o.reps)
    for m in (8, 4, 2, 1):                                           # (the largest of these sets whose blanket a factor holds)
        try:
            ms_marg, (fi, idx) = timed(lambda: g.marginalize(p, list(range(m))))
        except RuntimeError as e:
            emit(what="marginalize", removed=m, refused=int(e.args[0]))
            continue
        ms_cold, _ = timed(lambda: g.cholesky(p))
        emit(what="marginalize", removed=m, blanket=int(g.get_gaussian(fi)) if fi is not None else 0, ms_marginalize=round(ms_marg, 3), ms_next_cold_call=round(ms_cold, 3),
             not_spd=int(p.stats()["not_spd"]), poses_left=g.n_nodes)
        break
    p.destroy(); g.destroy()

    # one Gaussian factor on 11 nodes, the relative constraints of a star around its first node: on 11 consecutive poses ("local": what a
    # marginalisation leaves behind) and on poses 37 apart ("spread": 55 pair entries between distant poses, which change the elimination tree)
    node_sets = {"gaussian_local": list(range(100, 111)), "gaussian_spread": [100 + 37 * i for i in range(11)]}
    n = 33
    rng = np.random.default_rng(1)
    J = np.zeros((n - 3, n))
    for i in range(1, 11):
        J[3 * i - 3:3 * i, 0:3] = -np.eye(3); J[3 * i - 3:3 * i, 3 * i:3 * i + 3] = np.eye(3)
    Lam = J.T @ np.diag(rng.uniform(1, 50, n - 3)) @ J
    Lam = 0.5 * (Lam + Lam.T)
    order = ["plain"] + list(node_sets)
    res = {k: [] for k in order}
    for r in range(o.rounds):
        for tag in (order if r % 2 == 0 else order[::-1]):
            g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
            if tag != "plain":
                g.add_factor_gaussian(node_sets[tag], st[node_sets[tag]], np.zeros(n), Lam)
            _, ms = g.batch_resident(p, o.steps)
            res[tag].append(round(float(np.median(ms)), 5))
            p.destroy(); g.destroy()
    emit(what="resident", steps=o.steps, rounds=o.rounds, **{"ms_step_" + k: v for k, v in res.items()},
         **{"median_" + k: round(float(np.median(v)), 5) for k, v in res.items()})
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write("# tools/marginal_prior_time.py: aprilsam_amd_marginal_prior / aprilsam_amd_graph_marginalize on M3500 and the resident step with one 11-node\n"
                "# dense Gaussian factor; ms, wall clock of the Python call (one MI355X)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
