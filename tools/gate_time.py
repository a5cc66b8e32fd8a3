#!/usr/bin/env python3
"""Time aprilsam_amd_marginals_joint_any and aprilsam_amd_gate_xyt (path solves of the retained factor) for n = 1, 100 and 1 000
candidates on M3500 and the 10^5 / 10^6-pose lattices, with the peak working memory of the path solves; for M3500 also scipy's host
time for the same joint blocks (splu of the same system, then solves for the unit columns of the queried poses).

    python tools/gate_time.py [--cases m3500,lattice316,lattice1000] [--ns 1,100,1000] [--reps 5]

The candidates are the typical front-end batch: the newest pose against n random older ones.  One JSON line per (case, n): ms of the
first call after a solve (it also builds the host table of the factor's fronts), the median of the repeat calls, for joint_any and for
gate_xyt (which includes the path solves), the work buffer bytes, and the solver step's ms for scale."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arrays_for(lib, name):
    from aprilsam_amd import datasets
    if name == "m3500":
        return datasets.m3500_batch()
    if name.startswith("lattice"):
        return lib.lattice_arrays(int(name[7:]))
    raise ValueError(name)


def candidates(N, n, seed=0):
    rng = np.random.default_rng(seed)
    a = np.full(n, N - 1, np.int32)
    b = rng.choice(N - 1, n, replace=False).astype(np.int32)
    z = rng.normal(size=(n, 3))
    W = np.tile(np.diag([100.0, 100.0, 1000.0]).ravel(), (n, 1))
    return a, b, z, W


def scipy_ms(arr, lam, a, b):
    import scipy.sparse.linalg as sla
    from tests.support.selinv_model import sparse_system, system_blocks
    states, fa, fb, z, W = arr
    N = len(states)
    Aii, Aab = system_blocks(states, fa, fb, z, W, lam)
    A = sparse_system(Aii, Aab, fa, fb).tocsc()
    t0 = time.perf_counter()
    lu = sla.splu(A)
    nodes = np.unique(np.r_[a, b])
    E = np.zeros((3 * N, 3 * len(nodes)))
    for k, q in enumerate(nodes):
        E[3 * q:3 * q + 3, 3 * k:3 * k + 3] = np.eye(3)
    lu.solve(E)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice316,lattice1000")
    ap.add_argument("--ns", default="1,100,1000")
    ap.add_argument("--reps", type=int, default=5)
    o = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import host
    lib = host.SolverLib()
    for name in o.cases.split(","):
        arr = arrays_for(lib, name)
        N = len(arr[0])
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        g.cholesky(p)
        t0 = time.perf_counter(); g.cholesky(p); step_ms = (time.perf_counter() - t0) * 1e3
        for n in [int(x) for x in o.ns.split(",")]:
            a, b, z, W = candidates(N, n)
            g.set_all_states(arr[0], relinearize=True)
            g.cholesky(p)                                       # a new factor: the first call builds the front table again
            t0 = time.perf_counter(); g.marginals_joint_any(p, a, b); first = (time.perf_counter() - t0) * 1e3
            rep, gate = [], []
            for _ in range(o.reps):
                t0 = time.perf_counter(); g.marginals_joint_any(p, a, b); rep.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); g.gate_xyt(p, a, b, z, W); gate.append((time.perf_counter() - t0) * 1e3)
            out = dict(case=name, poses=N, candidates=n, ms_joint_any_first=round(first, 3), ms_joint_any=round(float(np.median(rep)), 3),
                       ms_gate_xyt=round(float(np.median(gate)), 3), ms_gate_xyt_all=[round(x, 3) for x in gate],
                       peak_work_bytes=int(lib.dll.aprilsam_amd_debug_path_solve_bytes(p.ptr)), ms_solver_step=round(step_ms, 3))
            if name == "m3500":
                out["scipy_splu_solves_ms"] = round(scipy_ms(arr, p.c.tikhanov, a, b), 3)
            print(json.dumps(out), flush=True)
        p.destroy(); g.destroy()


if __name__ == "__main__":
    main()
