#!/usr/bin/env python3
"""Time aprilsam_amd_optimize_lm against the plain resident Gauss-Newton step on M3500 and the 10^5 / 10^6-pose
lattices, and the time to convergence on M3500 (headings + N(0, 0.3^2)) against a host loop of april_graph_cholesky + april_graph_chi2
calls stopped by the same ftol.

    python tools/lm_time.py [--cases m3500,lattice317,lattice1000] [--iters 20] [--out profiles/lm_time.txt]

Per iteration: the difference of two runs of K1 and K2 iterations (set-up, plan and copies cancel), the stop tests disabled
(ftol = xtol = 0, lambda_max = inf); LM with the status polled every iteration (check_every 1) and once per run (check_every = K).  The
plain step: aprilsam_amd_resident_steps(K, asynchronous) + one sync, the same difference.  Wall clock around synchronised calls."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arrays_for(lib, name):
    from aprilsam_amd import datasets
    st, fa, fb, z, W = datasets.m3500_batch() if name == "m3500" else lib.lattice_arrays(int(name[7:]))
    sigma = 0.3 if name == "m3500" else 0.1
    st = st.copy(); st[:, 2] += np.random.default_rng(1).normal(0.0, sigma, len(st))
    return st, fa, fb, z, W


def lm_ms(lib, arr, K, check_every):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.optimize_lm(p, max_iters=1)                       # plan, capture, warm-up
    g.set_all_states(arr[0], relinearize=True)
    t0 = time.perf_counter()
    r = g.optimize_lm(p, max_iters=K, check_every=check_every, ftol=0.0, xtol=0.0, lambda_max=float("inf"))
    ms = (time.perf_counter() - t0) * 1e3
    p.destroy(); g.destroy()
    return ms, r["iterations"]


def plain_ms(lib, arr, K):
    d = lib.dll
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 1, 0); d.aprilsam_amd_resident_sync(g.ptr, p.ptr)
    t0 = time.perf_counter()
    d.aprilsam_amd_resident_steps(g.ptr, p.ptr, K, 0); d.aprilsam_amd_resident_sync(g.ptr, p.ptr)
    ms = (time.perf_counter() - t0) * 1e3
    d.aprilsam_amd_resident_end(g.ptr, p.ptr)
    p.destroy(); g.destroy()
    return ms


def per_iter(f, K1, K2, reps=3):
    a = min(f(K1) for _ in range(reps)); b = min(f(K2) for _ in range(reps))
    return (b - a) / (K2 - K1)


def convergence(lib, arr, ftol=1e-10):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.optimize_lm(p, max_iters=1); g.set_all_states(arr[0], relinearize=True)
    t0 = time.perf_counter(); r = g.optimize_lm(p); t_lm = (time.perf_counter() - t0) * 1e3
    p.destroy(); g.destroy()
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param(); p.c.tikhanov = 0.0
    g.cholesky(p); g.set_all_states(arr[0], relinearize=True)
    t0 = time.perf_counter()
    F, steps = g.chi2(), 0
    while steps < 100:
        g.cholesky(p); steps += 1
        Fn = g.chi2()
        if F - Fn <= ftol * abs(F):
            break
        F = Fn
    t_gn = (time.perf_counter() - t0) * 1e3
    p.destroy(); g.destroy()
    return r, t_lm, steps, t_gn, Fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice317,lattice1000")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_time.txt"))
    a = ap.parse_args()
    from aprilsam_amd import host
    lib = host.SolverLib()
    lines = ["# tools/lm_time.py: ms per iteration (difference of runs of K and 2K iterations, K = %d), MI355X" % a.iters,
             "# case            N        plain   lm(check 1)  ratio   lm(check K)  ratio"]
    K = a.iters
    for name in a.cases.split(","):
        arr = arrays_for(lib, name)
        reps = 1 if name == "lattice1000" else 3
        pl = per_iter(lambda k: plain_ms(lib, arr, k), K, 2 * K, reps)
        l1 = per_iter(lambda k: lm_ms(lib, arr, k, 1)[0], K, 2 * K, reps)
        lk = per_iter(lambda k: lm_ms(lib, arr, k, k)[0], K, 2 * K, reps)
        line = "%-12s %9d  %9.4f  %9.4f  %6.3fx  %9.4f  %6.3fx" % (name, len(arr[0]), pl, l1, l1 / pl, lk, lk / pl)
        print(line, flush=True); lines.append(line)
    if "m3500" in a.cases:
        r, t_lm, steps, t_gn, Fn = convergence(lib, arrays_for(lib, "m3500"))
        line = ("m3500 sigma 0.3 to convergence: LM %d iterations (status %d) %.2f ms, F %.6f; host loop cholesky + chi2 (tikhanov 0, same ftol) "
                "%d steps %.2f ms, chi2 %.6f" % (r["iterations"], r["status"], t_lm, r["F_final"], steps, t_gn, Fn))
        print(line, flush=True); lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
