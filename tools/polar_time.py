#!/usr/bin/env python3
"""Cost of the polar pre-pass: resident ms per Gauss-Newton step of M3500 with every loop closure (|a - b| > 1)
replaced by the range-bearing factor of its own xyt measurement, against the same graph with those closures as the plain xyt factors they
were.  The structure of the two systems is identical, so the difference is k_polar_slot.

    python tools/polar_time.py [--iters 20] [--repeats 5] [--out profiles/polar_time.txt]

One JSON line, appended to --out as well.  W of the range-bearing factor: diag(W_xx of the closure, W_tt of the closure) -- the values do
not change the cost.  Per-kernel times of k_polar_slot: run this under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def graphs(lib):
    from aprilsam_amd import abi, datasets
    states, fa, fb, z, W = datasets.m3500_batch()
    loop = (fb >= 0) & (np.abs(fa - fb) > 1)
    plain = lib.new_graph(); plain.build_from_arrays(states, fa, fb, z, W)
    keep = ~loop
    # (the closures go behind the other factors in BOTH graphs: the same factor order, the same plan)
    order = np.concatenate([np.nonzero(keep)[0], np.nonzero(loop)[0]])
    plain.destroy()
    plain = lib.new_graph(); plain.build_from_arrays(states, fa[order], fb[order], z[order], W[order])
    polar = lib.new_graph(); polar.build_from_arrays(states, fa[keep], fb[keep], z[keep], W[keep])
    for i in np.nonzero(loop)[0]:
        zz = [float(np.hypot(z[i, 0], z[i, 1])), float(np.arctan2(z[i, 1], z[i, 0]))]
        polar.add_factor_polar(abi.POLAR_RANGE_BEARING, int(fa[i]), int(fb[i]), zz, [W[i, 0], 0.0, 0.0, W[i, 8]])
    return plain, polar, int(loop.sum()), len(states), len(fa)


def resident_ms(lib, g, iters):
    p = lib.new_param()
    g.batch_resident(p, 2)                       # (plan, captures)
    st = g.states()
    _, ms = g.batch_resident(p, iters)
    g.set_all_states(st, relinearize=True)       # (every measurement starts from the same states)
    p.destroy()
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_time.txt"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import host
    lib = host.SolverLib()
    plain, polar, n_polar, N, F = graphs(lib)
    ms = dict(plain=[], polar=[])
    for _ in range(a.repeats):                   # (interleaved: a drift of the box's clocks hits both alike)
        ms["plain"].append(resident_ms(lib, plain, a.iters))
        ms["polar"].append(resident_ms(lib, polar, a.iters))
    mp, mq = float(np.median(ms["plain"])), float(np.median(ms["polar"]))
    line = json.dumps(dict(case="m3500", poses=N, factors=F, polar_factors=n_polar, iters=a.iters, repeats=a.repeats, ms_step_xyt=mp, ms_step_polar=mq,
                           ratio=mq / mp, overhead_pct=100.0 * (mq - mp) / mp, ms_step_xyt_runs=ms["plain"], ms_step_polar_runs=ms["polar"]))
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    plain.destroy(); polar.destroy()


if __name__ == "__main__":
    main()
