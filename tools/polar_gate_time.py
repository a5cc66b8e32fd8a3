#!/usr/bin/env python3
"""Time aprilsam_amd_associate_polar on M3500 with landmarks added by the model's generator
(tests/support/polar_model.with_landmarks): m = 32 observations from the newest pose against L = 1, 100 and 1 000 landmarks, and in the
same run, interleaved, aprilsam_amd_gate_xyt on the same L pairs -- the yardstick: the path solves are common to both -- and
aprilsam_amd_gate_polar on the m L expanded candidate list.

    python tools/polar_gate_time.py [--landmarks 1000] [--m 32] [--Ls 1,100,1000] [--reps 7] [--out profiles/polar_gate_time.txt]

One JSON line per L, appended to --out as well: the median ms of each call with every run, and the ratios to gate_xyt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def landmarks(pm, states, total, per=10, window=8, radius=6.0):
    """`total` landmarks along the trajectory: the model's generator on windows of `window` consecutive poses, `per` landmarks each, seen
    as range-bearing factors from the window's poses within `radius` (a seed whose landmarks are all seen is searched per window; the last
    window ends at the newest pose) -> (states with the landmarks appended, polars in the graph's ids)"""
    N = len(states)
    xs, polars = [states], []
    for w, s0 in enumerate(np.linspace(0, N - window, total // per).astype(int)):
        idx = np.arange(s0, s0 + window)
        for seed in range(100 * w, 100 * w + 100):
            try:
                _, x0, pl = pm.with_landmarks(states[idx], states[idx], per, radius=radius, seed=seed)
                break
            except AssertionError:          # (a landmark seen from nowhere)
                continue
        else:
            raise RuntimeError(f"no seed places the landmarks of window {w}")
        base = N + per * w
        xs.append(x0[window:])
        polars += [(k, int(idx[a]), base + (b - window), zz, WW) for k, a, b, zz, WW in pl]
    return np.vstack(xs), polars


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=1000)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--Ls", default="1,100,1000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_gate_time.txt"))
    o = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import abi, datasets, host
    from tests.support import polar_gate_model as pg
    from tests.support import polar_model as pm
    lib = host.SolverLib()
    states, fa, fb, z, W = datasets.m3500_batch()
    N = len(states)
    x0, polars = landmarks(pm, states, o.landmarks)
    g = pm.build(lib, x0, (fa, fb, z, W), polars); p = lib.new_param()
    g.cholesky(p)
    t0 = time.perf_counter(); g.cholesky(p); step_ms = (time.perf_counter() - t0) * 1e3
    assert p.stats()["not_spd"] == 0
    st = g.states()
    rng = np.random.default_rng(1)
    observer = N - 1
    order = N + np.argsort(np.hypot(*(st[N:, :2] - st[observer, :2]).T))          # the landmarks, the nearest to the observer first
    kinds = (abi.POLAR_RANGE_BEARING, abi.POLAR_RANGE, abi.POLAR_BEARING)
    obs = []
    for i in range(o.m):                                                          # readings of the nearest landmarks, the kinds cycling
        zz = pm.h(pm.RANGE_BEARING, pm.rel(st[observer], st[order[i % len(order)]])[0]) + rng.normal(0, [pm.SIGMA_RHO, pm.SIGMA_BETA])
        k = kinds[i % 3]
        obs.append((k, zz[:1], [1 / pm.SIGMA_RHO ** 2]) if k == abi.POLAR_RANGE else (k, zz[1:], [1 / pm.SIGMA_BETA ** 2]) if k == abi.POLAR_BEARING
                   else (k, zz, np.diag([1 / pm.SIGMA_RHO ** 2, 1 / pm.SIGMA_BETA ** 2])))
    kind, zp, Wp = host.polar_candidates(obs)
    for L in [int(x) for x in o.Ls.split(",")]:
        lms = np.ascontiguousarray(order[:L], np.int32)
        a = np.full(L, observer, np.int32)
        zx = rng.normal(size=(L, 3)); Wx = np.tile(np.diag([100.0, 100.0, 1000.0]).ravel(), (L, 1))
        ea = np.full(o.m * L, observer, np.int32); eb = np.tile(lms, o.m)
        ek, ez, eW = np.repeat(kind, L), np.repeat(zp, L, 0), np.repeat(Wp, L, 0)
        calls = dict(associate=lambda: g.associate_polar(p, observer, kind, zp, Wp, lms, pg.CHI2_1_999, pg.CHI2_2_999, matrix=False),
                     associate_matrix=lambda: g.associate_polar(p, observer, kind, zp, Wp, lms, pg.CHI2_1_999, pg.CHI2_2_999),
                     gate_xyt=lambda: g.gate_xyt(p, a, lms, zx, Wx),
                     gate_polar_expanded=lambda: g.gate_polar(p, ea, eb, ek, ez, eW))
        for f in calls.values():
            f()                                                                   # (buffers, the host table of the fronts)
        ms = {k: [] for k in calls}
        for _ in range(o.reps):                                                   # interleaved: a drift of the clocks hits all alike
            for k, f in calls.items():
                t0 = time.perf_counter(); f(); ms[k].append((time.perf_counter() - t0) * 1e3)
        r = calls["associate"]()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        line = json.dumps(dict(case="m3500+landmarks", poses=N, landmarks=o.landmarks, polar_factors=len(polars), m=o.m, L=L, reps=o.reps,
                               matched=int((r["best"] >= 0).sum()), ms_solver_step=round(step_ms, 3),
                               **{f"ms_{k}": round(v, 4) for k, v in med.items()},
                               ratio_associate_to_gate_xyt=round(med["associate"] / med["gate_xyt"], 3),
                               ratio_associate_matrix_to_gate_xyt=round(med["associate_matrix"] / med["gate_xyt"], 3),
                               ratio_gate_polar_expanded_to_gate_xyt=round(med["gate_polar_expanded"] / med["gate_xyt"], 3),
                               **{f"ms_{k}_runs": [round(x, 4) for x in v] for k, v in ms.items()}))
        print(line, flush=True)
        if o.out:
            os.makedirs(os.path.dirname(o.out), exist_ok=True)
            with open(o.out, "a") as f:
                f.write(line + "\n")
    p.destroy(); g.destroy()


if __name__ == "__main__":
    main()
