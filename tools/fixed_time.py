#!/usr/bin/env python3
"""Cost of the fixed-node mask: resident ms per Gauss-Newton step of M3500 with node 0 fixed against the same
graph with nobody fixed.  The plan is the same (a fixed node keeps its place in the ordering), so the difference is k_fix_mask: one launch
of one thread per record on the step's chain.

    python tools/fixed_time.py [--iters 20] [--repeats 5] [--fixed 0] [--out profiles/fixed_time.txt]

One JSON line, appended to --out as well.  --fixed takes a comma-separated list of node ids."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--fixed", default="0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixed_time.txt"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import datasets, host
    lib = host.SolverLib()
    states, fa, fb, z, W = datasets.m3500_batch()
    fixed = [int(v) for v in a.fixed.split(",") if v != ""]
    free = lib.new_graph(); free.build_from_arrays(states, fa, fb, z, W)
    held = lib.new_graph(); held.build_from_arrays(states, fa, fb, z, W)
    for i in fixed:
        assert held.set_fixed(i, True) == 0
    fx = np.zeros(len(states), bool); fx[fixed] = True
    records = int(np.sum(fx[fa] | ((fb >= 0) & fx[np.where(fb >= 0, fb, 0)])))
    ms = dict(free=[], fixed=[])
    for _ in range(a.repeats):                   # (interleaved: a drift of the box's clocks hits both alike)
        ms["free"].append(resident_ms(lib, free, a.iters))
        ms["fixed"].append(resident_ms(lib, held, a.iters))
    mf, mh = float(np.median(ms["free"])), float(np.median(ms["fixed"]))
    line = json.dumps(dict(case="m3500", poses=len(states), factors=len(fa), fixed_nodes=len(fixed), mask_records=records, iters=a.iters, repeats=a.repeats,
                           ms_step_free=mf, ms_step_fixed=mh, ratio=mh / mf, overhead_pct=100.0 * (mh - mf) / mf, ms_step_free_runs=ms["free"],
                           ms_step_fixed_runs=ms["fixed"]))
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    free.destroy(); held.destroy()


if __name__ == "__main__":
    main()
