#!/usr/bin/env python3
"""Cost of max-mixture factors: resident ms per Gauss-Newton step with and without them, and the total time of
M3500 grown pose by pose through april_graph_cholesky_inc with its loop closures as max factors or as plain xyt factors.

    python tools/maxmix_time.py [--cases m3500,lattice316,lattice1000,inc] [--iters 20]

One JSON line per case.  M3500: every loop closure (|a - b| > 1) becomes a 2-component factor {z, W, ln 0.9} / {z, 1e-6 W, ln 0.1}; the
lattices: every 10th edge.  Per-kernel times of k_select_mixture / k_chi2_mixture: run this under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def split(name, lib):
    from aprilsam_amd import datasets
    if name == "m3500":
        states, fa, fb, z, W = datasets.m3500_batch()
        mix = (fb >= 0) & (np.abs(fa - fb) > 1)
    else:
        states, fa, fb, z, W = lib.lattice_arrays(int(name[7:]))
        mix = np.zeros(len(fa), bool); mix[::10] = True; mix &= fb >= 0
    return states, fa, fb, z, W, mix


def resident_ms(lib, g, iters):
    p = lib.new_param()
    g.batch_resident(p, 2)                       # (plan, captures)
    _, ms = g.batch_resident(p, iters)
    p.destroy()
    return float(np.median(ms))


def inc_total_ms(lib, as_max):
    from aprilsam_amd import datasets
    from tests.support import maxmix_model as mm
    states, fa, fb, z, W = datasets.m3500_batch()
    order = np.argsort(np.maximum(fa, fb), kind="stable")
    g = lib.new_graph(); p = lib.new_param()
    k, t = 0, 0.0
    for n in range(len(states)):
        g.add_node_xyt(states[n])
        while k < len(order) and max(fa[order[k]], fb[order[k]]) <= n:
            i = order[k]; k += 1
            if fb[i] < 0:
                g.add_factor_xytpos(int(fa[i]), z[i], W[i].reshape(3, 3))
            elif as_max and abs(int(fa[i]) - int(fb[i])) > 1:
                g.add_factor_max(int(fa[i]), int(fb[i]), *mm.two_component(z[i], W[i]))
            else:
                g.add_factor_xyt(int(fa[i]), int(fb[i]), z[i], W[i].reshape(3, 3))
        t0 = time.perf_counter()
        if n == 10:
            g.cholesky(p)
        elif n > 10:
            p.c.batch_time = 1e300
            g.cholesky_inc(p)
        t += time.perf_counter() - t0
    p.destroy(); g.destroy()
    return t * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice316,lattice1000,inc")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import host
    from tests.support import maxmix_model as mm
    lib = host.SolverLib()
    for name in a.cases.split(","):
        if name == "inc":
            plain, mixed = inc_total_ms(lib, False), inc_total_ms(lib, True)
            print(json.dumps(dict(case="m3500_incremental", ms_total_plain=plain, ms_total_max=mixed)), flush=True)
            continue
        states, fa, fb, z, W, mix = split(name, lib)
        g = lib.new_graph(); g.build_from_arrays(states, fa, fb, z, W)
        plain = resident_ms(lib, g, a.iters)
        g.destroy()
        g = lib.new_graph(); g.build_from_arrays(states, fa[~mix], fb[~mix], z[~mix], W[~mix])
        for i in np.nonzero(mix)[0]:
            g.add_factor_max(int(fa[i]), int(fb[i]), *mm.two_component(z[i], W[i]))
        mixed = resident_ms(lib, g, a.iters)
        g.destroy()
        print(json.dumps(dict(case=name, poses=len(states), factors=len(fa), max_factors=int(mix.sum()), ms_step_plain=plain,
                              ms_step_max=mixed, overhead_pct=100.0 * (mixed - plain) / plain)), flush=True)


if __name__ == "__main__":
    main()
