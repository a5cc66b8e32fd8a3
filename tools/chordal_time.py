#!/usr/bin/env python3
"""Time aprilsam_amd_initialize_chordal on M3500 and the 10^5 / 10^6-pose lattices next to the plain resident
Gauss-Newton step.

    python tools/chordal_time.py [--cases m3500,lattice317,lattice1000] [--reps 20] [--plain-lib PATH] [--out profiles/chordal_time.txt]

The call: warm plan (one call before the timed ones), every call from all-zero states, wall clock around the synchronous call, median of
--reps.  The plain step: aprilsam_amd_resident_steps(K, asynchronous) + one sync, the difference of runs of K and 2K steps (tools/lm_time.py),
median of --reps differences; the api call: one synchronous april_graph_cholesky with a warm plan; --plain-lib measures it with another build of the library (the parent commit's) in the same session."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arrays_for(lib, name):
    from aprilsam_amd import datasets
    return datasets.m3500_batch() if name == "m3500" else lib.lattice_arrays(int(name[7:]))


def chordal_ms(lib, arr, reps):
    zero = np.zeros_like(arr[0])
    g = lib.new_graph(); g.build_from_arrays(zero, *arr[1:]); p = lib.new_param()
    g.initialize_chordal(p)                             # plan, warm-up
    ms = []
    for _ in range(reps):
        g.set_all_states(zero, relinearize=True)
        t0 = time.perf_counter()
        r = g.initialize_chordal(p)
        ms.append((time.perf_counter() - t0) * 1e3)
    p.destroy(); g.destroy()
    return float(np.median(ms)), float(np.min(ms)), r


def api_ms(lib, arr, reps):
    """one synchronous april_graph_cholesky call, warm plan: what packing, uploading and copying back cost around one step"""
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.cholesky(p); g.cholesky(p)
    ms = []
    for _ in range(reps):
        g.set_all_states(arr[0], relinearize=True)
        t0 = time.perf_counter()
        g.cholesky(p)
        ms.append((time.perf_counter() - t0) * 1e3)
    p.destroy(); g.destroy()
    return float(np.median(ms))


def plain_ms(lib, arr, K, reps):
    d = lib.dll
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 1, 0); d.aprilsam_amd_resident_sync(g.ptr, p.ptr)

    def run(k):
        t0 = time.perf_counter()
        d.aprilsam_amd_resident_steps(g.ptr, p.ptr, k, 0); d.aprilsam_amd_resident_sync(g.ptr, p.ptr)
        return (time.perf_counter() - t0) * 1e3

    ms = [(run(2 * K) - run(K)) / K for _ in range(reps)]
    d.aprilsam_amd_resident_end(g.ptr, p.ptr)
    p.destroy(); g.destroy()
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice317,lattice1000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--plain-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chordal_time.txt"))
    a = ap.parse_args()
    from aprilsam_amd import host
    lib = host.SolverLib()
    plib = host.SolverLib(a.plain_lib) if a.plain_lib else lib
    lines = ["# tools/chordal_time.py: aprilsam_amd_initialize_chordal from all-zero states, warm plan, median (min) of %d calls; the plain resident"
             % a.reps,
             "# step: difference of runs of K and 2K steps (K = %d), median of %d%s; ms, MI355X" % (a.steps, a.reps, ", the parent commit's build" if a.plain_lib else ""),
             "# api call: one synchronous april_graph_cholesky, warm plan, this build (host packing, upload and copy-back around one step)",
             "# case            N     chordal (min)        plain step   chordal / step    api call   F_initial -> F_final"]
    K = a.steps
    for name in a.cases.split(","):
        arr = arrays_for(lib, name)
        reps = max(3, a.reps // 4) if name == "lattice1000" else a.reps
        med, mn, r = chordal_ms(lib, arr, reps)
        pl = plain_ms(plib, arr, K, reps)
        api = api_ms(lib, arr, reps)
        line = "%-12s %9d  %9.3f (%9.3f)  %9.4f  %8.2fx  %9.3f   %.6g -> %.6g" % (name, len(arr[0]), med, mn, pl, med / pl, api, r["F_initial"], r["F_final"])
        print(line, flush=True); lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
