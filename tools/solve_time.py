#!/usr/bin/env python3
"""Time aprilsam_amd_solve (FULL, FORWARD, BACKWARD at nrhs 1, 3, 16, 64), aprilsam_amd_marginals_cross for all nodes and
aprilsam_amd_relative_covariances for all nodes (first call after a solver step, which runs the selected inversion, and a repeat call)
on M3500 and the 10^5 / 10^6-pose lattices: warm plan, repeat calls, the host's clock around the synchronous call.

    python tools/solve_time.py [--cases m3500,lattice316,lattice1000] [--nrhs 1,3,16,64] [--reps 5]

One JSON line per case.  Beside every figure, from the same run: the april_graph_cholesky step time, marginals_joint_any of the same
anchor (the newest pose) against 1 000 other poses, the peak work buffer (aprilsam_amd_debug_solve_bytes), and the floor of one pass:
stats.bytes_fronts read once at 8 TB/s, the HBM peak every roofline fraction of this project is taken against.
The backward error of the widest FULL solve is printed (computed on the host from the sparse system)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12          # "Peaks used for roofline fractions: HBM 8 TB/s"


def arrays_for(lib, name):
    from aprilsam_amd import datasets
    if name == "m3500":
        return datasets.m3500_batch()
    if name.startswith("lattice"):
        return lib.lattice_arrays(int(name[7:]))
    raise ValueError(name)


def timed(f, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice316,lattice1000")
    ap.add_argument("--nrhs", default="1,3,16,64")
    ap.add_argument("--reps", type=int, default=5)
    o = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import host
    from tests.support.selinv_model import sparse_system, system_blocks
    from tests.support.treesolve_model import backward_error
    lib = host.SolverLib()
    for name in o.cases.split(","):
        arr = arrays_for(lib, name)
        N = len(arr[0])
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        g.cholesky(p)
        step_ms = timed(lambda: g.cholesky(p), o.reps)           # (warm plan, like every figure below: the median of --reps calls)
        st = p.stats()
        out = dict(case=name, poses=N, ms_solver_step=step_ms, bytes_fronts=int(st["bytes_fronts"]),
                   ms_floor_one_pass=round(st["bytes_fronts"] / HBM_BYTES_PER_S * 1e3, 4))
        rng = np.random.default_rng(0)
        g.solve(p, rng.normal(size=3 * N))                      # (builds the tables of this factor)
        for nrhs in [int(x) for x in o.nrhs.split(",")]:
            B = rng.normal(size=(nrhs, 3 * N))
            for mode in ("full", "forward", "backward"):
                out[f"ms_{mode}_{nrhs}"] = timed(lambda: g.solve(p, B, mode), o.reps)
        X = g.solve(p, B)
        states, fa, fb, z, W = arr
        Aii, Aab = system_blocks(g.l_points(), fa, fb, z, W, p.c.tikhanov)
        out["omega_full"] = float(backward_error(sparse_system(Aii, Aab, fa, fb), X.T, B.T).max())
        del X, B
        anchor = N - 1
        out["ms_cross_all"] = timed(lambda: g.marginals_cross(p, anchor), o.reps)
        t0 = time.perf_counter(); g.relative_covariances(p, anchor); out["ms_relative_all_first"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["ms_relative_all"] = timed(lambda: g.relative_covariances(p, anchor), o.reps)
        b = rng.choice(N - 1, min(1000, N - 1), replace=False).astype(np.int32)
        a = np.full(len(b), anchor, np.int32)
        g.marginals_joint_any(p, a, b)
        out["ms_joint_any_1000"] = timed(lambda: g.marginals_joint_any(p, a, b), o.reps)
        out["peak_work_bytes"] = int(lib.dll.aprilsam_amd_debug_solve_bytes(p.ptr))
        print(json.dumps(out), flush=True)
        p.destroy(); g.destroy()


if __name__ == "__main__":
    main()
