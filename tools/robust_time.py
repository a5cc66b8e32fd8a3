#!/usr/bin/env python3
"""Cost of robust losses: resident ms per Gauss-Newton step of a graph with and without robust factors, and LM ms
per iteration on M3500.

    python tools/robust_time.py [--cases m3500,lattice316,lattice1000,lm] [--iters 20]

One JSON line per case.  M3500: every loop closure (|a - b| > 1) Cauchy, c = 1; the lattices: every 10th edge Cauchy, c = 1.  The weights
are 1 or below depending on the graph: the cost does not depend on them.  Per-kernel times of k_robust_weight / k_chi2_robust /
k_lm_cost_robust: run this under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def split(name, lib):
    from aprilsam_amd import datasets
    if name == "m3500":
        states, fa, fb, z, W = datasets.m3500_batch()
        rob = (fb >= 0) & (np.abs(fa - fb) > 1)
    else:
        states, fa, fb, z, W = lib.lattice_arrays(int(name[7:]))
        rob = np.zeros(len(fa), bool); rob[::10] = True; rob &= fb >= 0
    return states, fa, fb, z, W, rob


def graph(lib, states, fa, fb, z, W, rob):
    g = lib.new_graph(); g.build_from_arrays(states, fa, fb, z, W)
    for i in np.nonzero(rob)[0]:
        assert g.set_robust(int(i), 2, 1.0) == 0
    return g


def resident_ms(lib, g, iters):
    p = lib.new_param()
    g.batch_resident(p, 2)                       # (plan, captures)
    _, ms = g.batch_resident(p, iters)
    p.destroy()
    return float(np.median(ms))


def lm_ms(lib, g, x0, iters):
    """ms per LM iteration: a run of `iters` iterations (ftol / xtol 0: no early stop) minus a run of 1, from the same start"""
    import time
    out = []
    for n in (1, iters):
        p = lib.new_param()
        g.set_all_states(x0, relinearize=True)
        g.optimize_lm(p, max_iters=1)                # (plan, captures)
        g.set_all_states(x0, relinearize=True)
        t0 = time.perf_counter()
        r = g.optimize_lm(p, max_iters=n, ftol=0.0, xtol=0.0, check_every=n)
        out.append((time.perf_counter() - t0, r["iterations"]))
        p.destroy()
    return 1e3 * (out[1][0] - out[0][0]) / max(out[1][1] - out[0][1], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice316,lattice1000,lm")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import host
    lib = host.SolverLib()
    for name in a.cases.split(","):
        if name == "lm":
            from tests.support import lm_model
            states, fa, fb, z, W, rob = split("m3500", lib)
            x0 = lm_model.perturbed(states, 0.3)
            res = {}
            for tag, r in (("plain", np.zeros_like(rob)), ("robust", rob)):
                g = graph(lib, states, fa, fb, z, W, r)
                res[tag] = lm_ms(lib, g, x0, a.iters)
                g.destroy()
            print(json.dumps(dict(case="m3500_lm", robust_factors=int(rob.sum()), ms_iter_plain=res["plain"], ms_iter_robust=res["robust"],
                                  overhead_pct=100.0 * (res["robust"] - res["plain"]) / res["plain"])), flush=True)
            continue
        states, fa, fb, z, W, rob = split(name, lib)
        ms = {}
        for tag, r in (("plain", np.zeros_like(rob)), ("robust", rob)):
            g = graph(lib, states, fa, fb, z, W, r)
            ms[tag] = resident_ms(lib, g, a.iters)
            g.destroy()
        print(json.dumps(dict(case=name, poses=len(states), factors=len(fa), robust_factors=int(rob.sum()), ms_step_plain=ms["plain"],
                              ms_step_robust=ms["robust"], overhead_pct=100.0 * (ms["robust"] - ms["plain"]) / ms["plain"])), flush=True)


if __name__ == "__main__":
    main()
