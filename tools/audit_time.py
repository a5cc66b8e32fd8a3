#!/usr/bin/env python3
"""Time aprilsam_amd_factor_audit for ALL factors of M3500 and the 10^5 / 10^6-pose lattices.

    python tools/audit_time.py [--cases m3500,lattice316,lattice1000] [--reps 5] [--out profiles/factor_audit.txt] [--lib PATH --variant NAME]

One JSON line per case: ms of the param's very first call (buffers allocated), of the first call after the next solve (it includes
the selected inversion), the median of the repeat calls (kernel +
copy of 4 doubles per factor), and -- the yardstick, in the same run -- the repeat-call time of aprilsam_amd_marginals for all nodes,
which extracts 9 values per node from the same Sigma pool (the audit gathers 36 per factor, and there are about four factors per node).
The times are wall clock of the Python call: list building, copies and the kernel.  Kernel times come from a trace in a run of its own,
`rocprofv3 --kernel-trace --stats -- python tools/audit_time.py --cases lattice316` (profiles/factor_audit.txt quotes one).

--lib PATH --variant NAME: time another build of the library -- the one-thread form of k_factor_audit is the same source compiled with
-DAPRILSAM_AMD_AUDIT_LANES=1 (profiles/README.md has the commands) -- and mark its lines "variant": NAME.  The output file is not started
over: a line is replaced only by a new one of the same case and variant, and the comment lines (notes taken by hand, such as kernel times
from a trace) stay where they are."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gate_time import arrays_for      # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="m3500,lattice316,lattice1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_audit.txt"))
    ap.add_argument("--lib", default=None, help="another build of the library (default: the tree's, built first)")
    ap.add_argument("--variant", default=None, help="label of that build in the output lines")
    o = ap.parse_args()
    from aprilsam_amd import host
    if o.lib:
        lib = host.SolverLib(o.lib)
    else:
        import __graft_entry__ as ge
        ge.build()
        lib = host.SolverLib()
    lines = []
    for name in o.cases.split(","):
        arr = arrays_for(lib, name)
        N, F = len(arr[0]), len(arr[1])
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        g.cholesky(p)
        cold, _ = timed(lambda: g.factor_audit(p))             # (the param's first call also allocates the Sigma pool and the pinned result)
        step_ms, _ = timed(lambda: g.cholesky(p))
        first, (rows, _) = timed(lambda: g.factor_audit(p))
        rep = [timed(lambda: g.factor_audit(p))[0] for _ in range(o.reps)]
        marg = [timed(lambda: g.marginals(p))[0] for _ in range(o.reps)]
        out = dict(case=name, **({"variant": o.variant} if o.variant else {}), poses=N, factors=F, ms_audit_cold=round(cold, 3), ms_audit_first=round(first, 3), ms_audit_repeat=round(float(np.median(rep)), 3),
                   ms_audit_repeat_all=[round(x, 3) for x in rep], ms_marginals_repeat=round(float(np.median(marg)), 3),
                   ms_solver_step=round(step_ms, 3), below_checkability_1e3=int((rows[:, 3] < 1e-3).sum()))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        p.destroy(); g.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    key = lambda line: (json.loads(line)["case"], json.loads(line).get("variant"))
    new = {key(line): line for line in lines}
    old = open(o.out).read().splitlines() if os.path.exists(o.out) else ["# tools/audit_time.py: aprilsam_amd_factor_audit, all factors; ms, wall clock of the Python call"]
    kept = []
    for line in old:                                             # (a measured line takes the place of its predecessor; comments and the other lines stay)
        if line.startswith("{") and key(line) in new:
            line = new.pop(key(line))
        kept.append(line)
    last = max([i for i, line in enumerate(kept) if line.startswith("{")], default=0)
    kept[last + 1:last + 1] = list(new.values())
    with open(o.out, "w") as f:
        f.write("\n".join(kept) + "\n")


if __name__ == "__main__":
    main()
