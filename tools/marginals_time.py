#!/usr/bin/env python3
"""Time aprilsam_amd_marginals (all diagonal blocks) beside the solver step that made the factor, on M3500 and the 10^5 / 10^6-pose
lattices; scipy's CPU time for the same diagonal blocks as context (splu of the same system, then solves for the unit columns of
a sample of poses, extrapolated to all poses).

    python tools/marginals_time.py [--cases m3500,lattice316,lattice1000] [--reps 5] [--scipy-max 200000]

One JSON line per case: ms per call (first call after a solve = full selected inversion + extraction; later calls = extraction
only), ms per solver step (april_graph_cholesky, warm), the selected inversion's flop count, scipy's ms."""
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


def scipy_ms(arr, lam, sample=64):
    import scipy.sparse.linalg as sla
    from tests.support.selinv_model import sparse_system, system_blocks
    states, fa, fb, z, W = arr
    N = len(states)
    Aii, Aab = system_blocks(states, fa, fb, z, W, lam)
    A = sparse_system(Aii, Aab, fa, fb).tocsc()
    t0 = time.perf_counter()
    lu = sla.splu(A)
    t1 = time.perf_counter()
    poses = np.random.default_rng(0).choice(N, min(sample, N), replace=False)
    E = np.zeros((3 * N, 3 * len(poses)))
    for k, n in enumerate(poses):
        E[3 * n:3 * n + 3, 3 * k:3 * k + 3] = np.eye(3)
    lu.solve(E)
    t2 = time.perf_counter()
    return dict(scipy_factor_ms=(t1 - t0) * 1e3, scipy_all_diag_ms_extrapolated=(t1 - t0) * 1e3 + (t2 - t1) * 1e3 * N / len(poses))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice316,lattice1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-max", type=int, default=200000, help="skip scipy above this many poses")
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import host
    lib = host.SolverLib()
    for name in a.cases.split(","):
        arr = arrays_for(lib, name)
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        g.cholesky(p)
        full, extract, step = [], [], []
        for _ in range(a.reps):
            g.set_all_states(arr[0], relinearize=True)
            t0 = time.perf_counter(); g.cholesky(p); step.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); g.marginals(p); full.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); g.marginals(p); extract.append((time.perf_counter() - t0) * 1e3)
        st = p.stats()
        N = len(arr[0])
        out = dict(case=name, poses=N, fronts=st["n_fronts"], levels=st["n_levels"], bytes_sigma=st["bytes_fronts"],
                   ms_marginals_full=float(np.median(full)), ms_marginals_extract=float(np.median(extract)),
                   ms_solver_step=float(np.median(step)), ms_marginals_full_all=[round(x, 3) for x in full])
        if N <= a.scipy_max:
            out.update(scipy_ms(arr, p.c.tikhanov))
        print(json.dumps(out), flush=True)
        p.destroy(); g.destroy()


if __name__ == "__main__":
    main()
