#!/usr/bin/env python3
"""Time the information measures on M3500, the 10^5-pose lattice and the 10^6-pose lattice, by hand on a GPU box:

    python tools/info_measure_times.py [--cases m3500,lattice316,lattice1000] [--reps 5] [--out profiles/info_measures.txt]

Every case runs in a child process of its own under a time limit (--limit seconds); a case that fails or runs out of time ends the run:
nothing more is started on the device after it.  One JSON line per figure, appended to --out:

* aprilsam_amd_logdet: the first call after a solve (it builds and uploads the table of (front, chunk) entries), the median of the repeat
  calls, beside one batch API call;
* aprilsam_amd_logdet_sets for 100 and 1 000 sets of 4 and 16 nodes around the newest pose (the 40 nodes of tools/joint_gate_time.py's
  pool), beside aprilsam_amd_marginals_set of the same sets, one call each, plus numpy's slogdet of every prefix on the host;
* aprilsam_amd_info_gain_xyt for the 100 x 4 / 100 x 16 / 1 000 x 4 / 1 000 x 16 hypotheses of profiles/joint_gate.txt, beside
  aprilsam_amd_gate_xyt_joint on the same hypotheses (no C matrices requested)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gate_time import arrays_for  # noqa: E402
from tools.joint_gate_time import hypotheses, pool_of, timed  # noqa: E402


def node_sets(states, n_sets, k, seed=0):
    rng = np.random.default_rng(seed)
    pa, pb = pool_of(states)
    pool = np.unique(np.r_[pa, pb])
    return [rng.choice(pool, k, replace=False).astype(np.int32) for _ in range(n_sets)]


def one_case(name, reps):
    import __graft_entry__ as ge
    ge.build()
    from aprilsam_amd import host
    from aprilsam_amd.host import _np_d, _np_i
    lib = host.SolverLib()
    arr = arrays_for(lib, name)
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.cholesky(p)
    t0 = time.perf_counter(); g.cholesky(p); step_ms = round((time.perf_counter() - t0) * 1e3, 3)
    st = g.states()
    base = dict(case=name, poses=len(st), ms_solver_step=step_ms)
    first, med = timed(lambda: g.logdet(p), reps)
    yield dict(base, call="logdet", logdet=g.logdet(p), ms_first=first, ms=med)
    for n_sets in (100, 1000):
        for k in (4, 16):
            sets = node_sets(st, n_sets, k)
            ptr = np.arange(0, n_sets * k + 1, k, dtype=np.int32); nodes = np.ascontiguousarray(np.concatenate(sets)); out = np.empty(n_sets * k)

            def dev():
                rc = lib.dll.aprilsam_amd_logdet_sets(g.ptr, p.ptr, n_sets, _np_i(ptr), _np_i(nodes), _np_d(out))
                assert rc == 0, (rc, lib.last_error())

            def hostside():
                for s in sets:
                    M = g.marginals_set(p, s)
                    for j in range(1, k + 1):
                        np.linalg.slogdet(M[:3 * j, :3 * j])
            g.cholesky(p)
            f, m = timed(dev, reps)
            _, hm = timed(hostside, 1)
            yield dict(base, call="logdet_sets", sets=n_sets, nodes_each=k, ms_first=f, ms=m, ms_marginals_set_and_host_slogdet=hm)
    for n_hyp in (100, 1000):
        for m_ in (4, 16):
            hyps = hypotheses(st, n_hyp, m_)
            a, b, z, W = (np.ascontiguousarray(np.concatenate([h[i] for h in hyps])) for i in range(4))
            ptr = np.arange(0, n_hyp * m_ + 1, m_, dtype=np.int32); out = np.empty(n_hyp * m_)

            def gain():
                rc = lib.dll.aprilsam_amd_info_gain_xyt(g.ptr, p.ptr, n_hyp, _np_i(ptr), _np_i(a), _np_i(b), _np_d(W), _np_d(out))
                assert rc == 0, (rc, lib.last_error())

            def gate():
                rc = lib.dll.aprilsam_amd_gate_xyt_joint(g.ptr, p.ptr, n_hyp, _np_i(ptr), _np_i(a), _np_i(b), _np_d(z), _np_d(W), _np_d(out), None)
                assert rc == 0, (rc, lib.last_error())
            g.cholesky(p)
            f, m = timed(gain, reps)
            _, gm = timed(gate, reps)
            yield dict(base, call="info_gain_xyt", hypotheses=n_hyp, candidates_each=m_, ms_first=f, ms=m, ms_gate_xyt_joint=gm)
    p.destroy(); g.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice316,lattice1000")
    ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=400, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "info_measures.txt"))
    o = ap.parse_args()
    if o.case:
        for row in one_case(o.case, o.reps):
            print(json.dumps(row), flush=True)
        return 0
    with open(o.out, "a") as f:
        for name in [c for c in o.cases.split(",") if c]:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(o.reps)], capture_output=True, text=True, timeout=o.limit)
            except subprocess.TimeoutExpired:
                print(f"{name}: no result within {o.limit} s; nothing more is started", file=sys.stderr)
                return 1
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            for ln in lines:
                print(ln, flush=True); f.write(ln + "\n")
            f.flush()
            if r.returncode != 0:
                print(f"{name}: exit status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
