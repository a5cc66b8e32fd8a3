#!/usr/bin/env python3
"""aprilsam_amd_optimize_gnc on M3500 with 50 false loop closures (tests/support/maxmix_model.m3500_outliers), from
chordal initialisation, Geman-McClure and truncated least squares, next to plain LM from the same start.  Run by hand on a GPU:

    python tools/gnc_m3500.py [--n_out 50] [--out profiles/gnc_m3500.txt]

Per run: stages, LM iterations, wall-clock time of the call (warm plan), true closures kept (s <= c^2) and false closures rejected.  Per
iteration: the call's time over its iterations, next to a plain LM iteration on the same graph (the difference of runs of K and 2K
iterations with the stop tests disabled, as tools/lm_time.py), same box, same build."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_out", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnc_m3500.txt"))
    a = ap.parse_args()
    from aprilsam_amd import abi, host
    from tests.support import robust_model
    lib = host.SolverLib()
    states, plain, _, _, n_base, n_loops = robust_model.m3500_robust(abi.ROBUST_NONE, 0.0, a.n_out)
    F = len(plain[0])
    cand = np.arange(n_base, F, dtype=np.int32)
    is_false = np.arange(n_base, F) >= n_base + n_loops

    def fresh():
        g = lib.new_graph(); g.build_from_arrays(np.zeros_like(states), *plain); p = lib.new_param()
        g.initialize_chordal(p)
        return g, p, g.states().copy()

    lines = ["# tools/gnc_m3500.py: M3500 + %d false loop closures, start = chordal initialisation, MI355X" % a.n_out]
    g, p, x0 = fresh()
    K = a.iters

    def lm_ms(k):
        g.set_all_states(x0, relinearize=True)
        t0 = time.perf_counter()
        g.optimize_lm(p, max_iters=k, ftol=0.0, xtol=0.0, lambda_max=float("inf"))
        return (time.perf_counter() - t0) * 1e3

    lm_ms(1)
    lm_it = (min(lm_ms(2 * K) for _ in range(3)) - min(lm_ms(K) for _ in range(3))) / K
    g.set_all_states(x0, relinearize=True)
    t0 = time.perf_counter(); r = g.optimize_lm(p); t = (time.perf_counter() - t0) * 1e3
    line = "plain LM: status %d, %d iterations, %.2f ms, F %.6g; %.4f ms per iteration" % (r["status"], r["iterations"], t, r["F_final"], lm_it)
    print(line, flush=True); lines.append(line)
    x_lm = g.states().copy()
    p.destroy(); g.destroy()
    for name, loss in (("GM", abi.GNC_GM), ("TLS", abi.GNC_TLS)):
        g, p, x0 = fresh()
        g.optimize_gnc(p, cand, loss=loss, max_stages=1)           # plan, capture, warm-up
        best = None
        for _ in range(3):
            g.set_all_states(x0, relinearize=True)
            t0 = time.perf_counter(); r = g.optimize_gnc(p, cand, loss=loss); t = (time.perf_counter() - t0) * 1e3
            best = t if best is None else min(best, t)
        inl = robust_model.s_of(g.states(), plain)[cand] <= 16.27
        line = ("GNC %-3s: status %d, %d stages, %d iterations (%d stages stalled), %.2f ms = %.4f ms per iteration (%.2fx a plain LM iteration); "
                "true closures kept %d / %d, false closures rejected %d / %d, largest weight of a false closure %.3g; F %.6g, chi2 %.6g; "
                "max |x - x_LM| %.3g" % (name, r["status"], r["stages"], r["iterations"], r["stages_stalled"], best, best / r["iterations"],
                                         best / r["iterations"] / lm_it, int(inl[~is_false].sum()), int((~is_false).sum()),
                                         int((~inl[is_false]).sum()), int(is_false.sum()), r["weights"][is_false].max(), r["F_final"],
                                         r["chi2_final"], np.abs(g.states()[:, :2] - x_lm[:, :2]).max()))
        print(line, flush=True); lines.append(line)
        p.destroy(); g.destroy()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
