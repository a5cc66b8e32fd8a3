#!/usr/bin/env python3
"""bench.py — BASELINE.json metric on MI355X: Gauss-Newton iterations/s (+ factorise ms) on M3500, chi^2 matched.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]     (N > 1 is launched by torch.distributed.run)

A plain run sets up, warms up (W steps), times K steps, writes what they left (--dump-outputs) and prints ONE JSON line with the contract
fields and `config`.  Everything else below -- the parity gate, the instrumented pass and `roofline`, the API-call figures, the CPU
baseline, the lattices, the incremental demo and the side file -- runs only with --full.

A "step" is one batch Gauss-Newton iteration of the hot path (relinearise -> linearise -> assemble ->
factorise -> solve -> update) over the whole M3500 graph (3500 poses, 5453 xyt factors + the prior), with
the node states and factor data already resident in HBM when the timed region starts; chi^2 is evaluated
outside the timed region, as examples/aprilsam_demo.c:103-107,229 does.  M3500 is far too small to shard
("replicas only"), so with N GPUs every rank solves its own replica: weak scaling,
value = N * K / max-over-ranks wall time.

`value` follows the bench contract to the letter: inputs resident in HBM when the timed region starts.  SURVEY.md
section 8(d) defines the metric one level further out -- one april_graph_cholesky call through the C-ABI, host objects in,
states valid in the host objects on return -- and that number stands right beside it: `value_api_call` /
`ms_per_api_call` (the same K steps as K warm API calls inside the same barrier + synchronize brackets, max over ranks);
`speedup_vs_cpu_baseline` is computed from the API number, because the reference's figure is a whole call too.

With --full, rank 0's ONE JSON line carries the contract fields plus
  roofline     — dominant kernel (by HIP-event time) of an instrumented pass of the same K steps: every
                 kernel launch bracketed by an event pair on the solver's own stream
  cpu_baseline — the reference CPU path (oracle/_ref, unmodified AprilSAM built from source) or, if it
                 did not travel, the C port (oracle/liboracle.so), timed on this box's host, 1 thread
  (everything below is NESTED and goes to the side file bench_extras.json + stderr, not to the stdout line: short_line / write_extras)
  parity       — max relative chi^2 error of 10 iterations vs the reference golden (tests/golden)
  lattice100k  — config 4 (99 856 poses) ms/iteration measured the same way, for BASELINE.md's second target
  lattice1m    — config 5 (10^6 poses, 3 994 003 factors): at N = 1 the single-GPU time per iteration; at N > 1 the SAME
                 graph solved once by all N ranks together — nested-dissection subtrees sharded over the ranks
                 (aprilsam_amd/shard.py), Schur slabs and separator solutions exchanged over RCCL — i.e. strong scaling
                 of one solve, reported beside (never instead of) the replica throughput that is `value`.  A watchdog
                 prints the line without this extra if the exchange does not finish in time.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6     # MI355X FP64 vector = matrix peak; HBM peak from MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0
PMC_TAG = "r06"              # profiles/<tag>_pmc_*.json written by tools/profile_round.sh <tag>
FLOP_KERNELS = {"k_front_small", "k_syrk_big", "k_panel_big"}
FACTOR_KERNELS = ("k_front_small", "k_assemble_big", "k_panel_big", "k_syrk_big")      # profile slots of the factorisation (k_panel_big = k_block_chain + k_block_solve)


def kernel_profile(lib, p):
    ms = (C.c_double * 16)(); calls = (C.c_longlong * 16)(); fl = (C.c_double * 16)(); by = (C.c_double * 16)()
    names = (C.c_char_p * 16)()
    n = lib.dll.aprilsam_amd_kernel_profile(p.ptr, ms, calls, fl, by, names)
    return [dict(name=names[k].decode(), ms=ms[k], calls=calls[k], flops=fl[k], bytes=by[k]) for k in range(n)]


HASHED_SOURCES = ("kernels.hip.h", "solver.hip.cpp", "solver_pack.inc.h", "solver_context.inc.h", "solver_inc.inc.h", "solver_calls.inc.h",
                  "solver_resident.inc.h", "solver_shard.inc.h")      # the kernels and the host runtime that launches them


def source_hash():
    """sha256[:16] of the kernel + host runtime sources: profiles/*_pmc_*.json carry the hash they were collected with"""
    import hashlib
    h = hashlib.sha256()
    for f in HASHED_SOURCES:
        h.update(open(os.path.join(ROOT, "aprilsam_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def load_pmc(name):
    """committed PMC summary (separate rocprofv3 --pmc passes, tools/profile_round.sh) -- refused when it was collected
    with other kernel sources than the ones this bench is running (stale counters are worse than none)"""
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", name)))
    except Exception:
        return None, "not collected"
    if d.get("source_hash") != source_hash():
        return None, f"stale: collected for sources {d.get('source_hash')}, running {source_hash()}"
    return d, f"profiles/{name}"


def survey_assembly_bytes(n_nodes, n_binary, n_unary):
    """SURVEY.md section 8(d), "Assembly bytes": factor records + poses read, upper triangle of A + B written, states read"""
    return n_binary * 152.0 + n_unary * 124.0 + 8.0 * (6 * n_nodes + 9 * n_binary) + 2 * 8.0 * 3 * n_nodes


def pmc_traffic(pmc, kernel):
    """HBM bytes per launch of `kernel` from a committed FETCH_SIZE / WRITE_SIZE pass pair: (2 x FETCH + WRITE) KB -- the x2 on
    the read side is the gfx950 correction of MI355X_MICROARCH.md (calibrated there for wide coalesced reads)"""
    try:
        cn = pmc["counters"]
        return 1024.0 * (2.0 * cn["FETCH_SIZE"][kernel]["kb_per_dispatch"] + cn["WRITE_SIZE"][kernel]["kb_per_dispatch"])
    except Exception:
        return None


# rocprofv3 kernel names of the K_BACKSOLVE / K_PANEL_BIG slots (several kernels share a slot)
PMC_NAMES = {"k_linearize": ("k_linearize_t",), "k_backsolve": ("k_backsolve_blk", "k_backsolve_t", "k_backsolve_w", "k_backsolve_gemv"), "k_panel_big": ("k_block_chain", "k_block_solve"),
             "k_syrk_big": ("k_syrk_big", "k_syrk_big32")}


def hbm_rooflines(prof, iters, pmc_file=None, survey_bytes=None):
    """roofline entries of the bandwidth-bound kernels from an instrumented pass of `iters` iterations: algorithmic bytes
    (SURVEY.md section 8(d) conventions, aprilsam_amd_kernel_profile) / HIP-event time; `traffic` per launch from the committed
    counter passes of the same workload"""
    pmc, src = load_pmc(pmc_file) if pmc_file else (None, "not collected")
    out = []
    # (k_front_small appears under both bounds: on the lattices' throughput levels -- thousands of leaves -- it streams the fronts through
    # HBM, near the top of a tree it is a latency chain; its bytes: each small front's L panel + update block once)
    for name in ("k_linearize", "k_assemble_big", "k_backsolve", "k_front_small"):
        k = next((q for q in prof if q["name"] == name), None)
        if not k or k["ms"] <= 0 or k["bytes"] <= 0:
            continue
        ach = k["bytes"] / (k["ms"] / iters * 1e-3) / 1e9
        e = dict(kernel=name, bound="hbm", achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach / HBM_PEAK_GBS,
                 algorithmic_bytes_per_step=k["bytes"], kernel_ms_per_step=k["ms"] / iters, launches_per_step=k["calls"] / iters)
        if name == "k_linearize" and survey_bytes:
            # the library's own count includes the 33-double contribution blocks it writes per factor (its design); SURVEY 8(d)'s
            # formula for linearise + assemble counts the assembled upper triangle instead
            e["survey_8d_bytes_per_step"] = survey_bytes
            e["frac_by_survey_8d_bytes"] = survey_bytes / (k["ms"] / iters * 1e-3) / 1e9 / HBM_PEAK_GBS
        tr = [(pmc_traffic(pmc, n), pmc["counters"]["FETCH_SIZE"].get(n, {}).get("dispatches", 0)) for n in PMC_NAMES.get(name, (name,))] if pmc else []
        tr = [(t, d) for t, d in tr if t]
        e["traffic"] = sum(t * d for t, d in tr) / max(1, sum(d for _, d in tr)) if tr else None      # bytes per launch, averaged over the slot's kernels
        # ... and per Gauss-Newton iteration of the profiled run (k_linearize runs once per iteration), next to the algorithmic bytes per step
        try:
            n_it = pmc["counters"]["FETCH_SIZE"]["k_linearize_t"]["dispatches"]
            e["traffic_per_step"] = sum(t * d for t, d in tr) / n_it if tr else None
            e["traffic_over_algorithmic"] = e["traffic_per_step"] / k["bytes"] if tr else None
        except Exception:
            pass
        e["traffic_source"] = src
        out.append(e)
    return out


def big_front_rooflines(prof, iters, pmc_file):
    """roofline entries of the wide-supernode path from an instrumented pass of `iters` iterations: k_syrk_big (its own tiles
    only: lower trapezoid right of every outer block) and the panel kernel (diagonal blocks, row solves, left-looking products)"""
    pmc, src = load_pmc(pmc_file)
    out = []
    for name in ("k_front_small", "k_syrk_big", "k_panel_big"):
        k = next((q for q in prof if q["name"] == name), None)
        if not k or k["ms"] <= 0 or k["flops"] <= 0:
            continue
        ach = k["flops"] / (k["ms"] / iters * 1e-3) / 1e12
        e = dict(kernel=name, bound="mfma", achieved=ach, peak=FP64_PEAK_TFLOPS, unit="TFLOP/s", frac=ach / FP64_PEAK_TFLOPS,
                 kernel_ms_per_step=k["ms"] / iters, launches_per_step=k["calls"] / iters, algorithmic_flops_per_step=k["flops"])
        if pmc:
            # one v_mfma_f64_16x16x4_f64 = 2048 flops = 4 "MOPS" units of 512: executed (incl. the discarded upper halves of
            # diagonal tiles) vs algorithmic, over all kernels of the slot (e.g. the 64 x 64 and the 32 x 32 tile forms of the wide update)
            cs = [pmc["kernels"][n] for n in PMC_NAMES.get(name, (name,)) if pmc["kernels"].get(n, {}).get("SQ_INSTS_VALU_MFMA_MOPS_F64")]
            if cs:
                nd = sum(c["dispatches"] for c in cs)
                e["mfma_executed_flops_per_dispatch"] = 512.0 * sum(c["SQ_INSTS_VALU_MFMA_MOPS_F64"] for c in cs) / max(1, nd)
                e["cus_busy_on_average"] = round(sum((c.get("cus_busy_on_average") or 0) * c["dispatches"] for c in cs) / max(1, nd), 2)
        e["counter_source"] = src
        out.append(e)
    return out


def level_profile(lib, p, iters):
    """per level of the assembly tree, from the instrumented pass (aprilsam_amd_level_profile): ms per iteration of the
    factorisation and of the back substitution, fronts, fronts on the multi-workgroup path, widest own part, GFLOP"""
    lv = (C.c_double * (6 * 64))()
    lib.dll.aprilsam_amd_level_profile.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    nl = lib.dll.aprilsam_amd_level_profile(C.cast(p.ptr, C.c_void_p), lv, 64)
    return [dict(level=l, factor_ms=lv[6 * l] / iters, backsolve_ms=lv[6 * l + 1] / iters, fronts=int(lv[6 * l + 2]), multi_workgroup=int(lv[6 * l + 3]),
                 widest_own_columns=int(lv[6 * l + 4]), gflop=lv[6 * l + 5] / 1e9) for l in range(max(nl, 0))]


def modelled_scaling_from_level_times(levels, other_ms, total_ms, chain_us_per_outer_block=80.0):
    """What the MEASURED single-GPU level times say about G GPUs (a model, labelled as such: this builder has one GPU).
    A level with n fronts takes t on one GPU; on G GPUs with the fronts spread over the ranks it takes t / min(n, G) -- but never
    less than the dependent chain of its widest front: one outer block of 128 columns after the other, ~80 us each (k_block_chain
    + k_block_solve + the wide update's launch; profiles/r03_chain_times_lattice100k.txt), which no amount of GPUs shortens.
    `owner`: a front whose rank range spans several ranks runs on ONE of them (what is built); `spread`: its trailing updates
    are shared by all ranks of its range, its panel chain is not (what SURVEY 8(e)'s block-cyclic top fronts could reach at
    best, before any communication).  Everything that is not a level kernel (linearisation, state update) is divided by G."""
    out = {}
    for G in (2, 4, 8):
        t_owner = t_spread = 0.0
        for L in levels:
            n = max(1, L["fronts"])
            chain = 1e-3 * chain_us_per_outer_block * ((L["widest_own_columns"] + 127) // 128) if L["multi_workgroup"] else 0.0
            both = L["factor_ms"] + L["backsolve_ms"]
            t_owner += max(chain, both / min(n, G))
            t_spread += max(chain, both / G)
        t_owner += other_ms / G; t_spread += other_ms / G
        out[f"G{G}"] = {"ms_top_fronts_on_one_owner": t_owner, "speedup_top_fronts_on_one_owner": total_ms / t_owner,
                        "ms_top_fronts_spread": t_spread, "speedup_top_fronts_spread": total_ms / t_spread}
    out["note"] = ("model from the measured per-level times of THIS single-GPU run (no communication, perfect balance below the top): "
                   "t_level / min(fronts, G), floored by the widest front's chain of 128-column outer blocks; 'spread' = the best a "
                   "distribution of the multi-rank fronts' updates could do")
    return out


def timed_steps(lib, g, p, K, sync_all, barrier):
    import torch
    barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    lib.dll.aprilsam_amd_resident_steps(g.ptr, p.ptr, K, 0)
    rc = lib.dll.aprilsam_amd_resident_sync(g.ptr, p.ptr)
    torch.cuda.synchronize(); barrier()
    t1 = time.perf_counter()
    assert rc == 0, "not positive definite"
    return sync_all(t1 - t0)


def cpu_baseline(arrays, budget_s=12.0):
    """reference CPU april_graph_cholesky on this host, single thread; bounded sample of whole iterations"""
    from aprilsam_amd import host
    from tests.support.oracle_binding import REFLIB, Oracle
    if os.path.exists(REFLIB):
        ref = host.SolverLib(REFLIB)
        g = ref.new_graph(); g.build_from_arrays(*arrays); p = ref.new_param()
        g.cholesky(p)                                     # warm-up (first call also pays page faults)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget_s or n < 3:
            g.cholesky(p); n += 1
        dt = time.perf_counter() - t0
        p.destroy(); g.destroy()
        kind = "reference"
    else:
        orc = Oracle()
        s, fa, fb, z, W = arrays
        s = np.array(s, float)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget_s or n < 3:
            s, _, _ = orc.batch_step(s, fa, fb, z, W); n += 1
        dt = time.perf_counter() - t0
        kind = "port"
    return dict(value=n / dt, unit="GN iterations/s", cores=1, kind=kind, ms_per_iter=1e3 * dt / n,
                sample=f"{n} consecutive batch iterations of the same M3500 graph ({dt:.1f} s of CPU time), "
                       f"wall clock around the solver call only")


def api_calls(lib, arrays, K=60, colds=5):
    """the metric as the reference's harness sees it (examples/aprilsam_demo.c:103-107) -- one
    april_graph_cholesky call through the C-ABI, host node / factor objects in, states valid in the host objects out.
    warm = the topology is unchanged since the previous call (ordering + symbolic plan cached);
    cold = the first call on a topology (host packing + nested dissection + symbolic + plan upload + numeric), what every
    step of the demo's --batch_update_only mode pays."""
    def med(xs):
        return float(np.median(np.asarray(xs, float)))
    out = {}
    for trust in (0, 1):
        lib.set_option("trust_factor_cache", trust)
        g = lib.new_graph(); g.build_from_arrays(*arrays); p = lib.new_param()
        t0 = time.perf_counter(); g.cholesky(p); cold = (time.perf_counter() - t0) * 1e3
        for _ in range(5):
            g.cholesky(p)
        wall, split = [], []
        for _ in range(K):
            t0 = time.perf_counter(); g.cholesky(p); wall.append((time.perf_counter() - t0) * 1e3)
            st = p.stats()
            split.append([st["ms_pack"], st["ms_symbolic"], st["ms_h2d"], st["ms_device"], st["ms_unpack"], st["ms_total"]])
        split = np.array(split)
        key = "default" if trust == 0 else "trust_factor_cache"
        out[key] = {"warm_ms_per_call": med(wall), "warm_calls": K, "warm_it_per_s": 1e3 / med(wall),
                    "split_ms": {"pack_host_objects": med(split[:, 0]), "plan_check": med(split[:, 1]), "upload": med(split[:, 2]),
                                 "device_incl_pinned_io_and_sync": med(split[:, 3]), "write_back_host_objects": med(split[:, 4]),
                                 "total_inside_library": med(split[:, 5])},
                    "first_call_ms": cold}
        p.destroy(); g.destroy()
    lib.set_option("trust_factor_cache", 0)
    cold = []
    for _ in range(colds):          # a fresh param (= no cached plan) on a warm process
        g = lib.new_graph(); g.build_from_arrays(*arrays); p = lib.new_param()
        t0 = time.perf_counter(); g.cholesky(p); cold.append((time.perf_counter() - t0) * 1e3)
        st = p.stats()
        p.destroy(); g.destroy()
    out["cold_ms_per_call"] = med(cold)
    out["cold_split_ms"] = {"pack": st["ms_pack"], "ordering_symbolic_plan_upload": st["ms_symbolic"], "upload": st["ms_h2d"],
                            "device": st["ms_device"], "write_back": st["ms_unpack"]}
    out["note"] = ("one april_graph_cholesky call through the C-ABI: host objects in, states valid in the host objects on return; "
                   "default = every factor object re-read and compared on every call (reference semantics), "
                   "trust_factor_cache = z/W of already packed factors treated as immutable")
    return out


def setup_dist(world, backend, device):
    """One process per GPU (launched by torch.distributed.run): returns (barrier, max_over_ranks).
    Replicas only — there is no data-path collective; the two helpers bracket the timed region and take the
    max wall time over ranks.  `backend` is "nccl" (= RCCL) on the GPU box, "gloo" in the CPU tests."""
    if world <= 1:
        return (lambda: None), (lambda dt: dt)
    import torch
    import torch.distributed as dist
    if not dist.is_initialized():
        kw = {"device_id": device} if backend == "nccl" else {}
        dist.init_process_group(backend, **kw)
    dist.barrier()

    def max_over_ranks(dt):
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())
    return dist.barrier, max_over_ranks


# chi^2 of the 1000 x 1000 lattice at the generator's initial states and after 1 / 2 Gauss-Newton iterations, from the
# single-GPU path (profiles/r01_lattice1m.json); the sharded solve must reproduce them
LATTICE1M_CHI2 = [236446240.54074645, 4636226.273819329, 4491095.9102143]      # after 0, 1 and 3 iterations


LATTICE100K_CHI2 = [23540091.69690116, 460825.57393385]


def normal_eq_check(lib, g, K):
    """parity property that needs no recorded trace (tests/support/normal_eq.py, a numpy checker pinned on the CPU against the oracle and
    the unmodified reference): the LAST iteration's dx, as resident_end left it in the node objects next to its linearisation point,
    against the reference's normal equations (J'WJ + lambda I) dx = J'W r -- outside every timed region"""
    from tests.support.normal_eq import normal_equation_residual
    arr = lib.lattice_arrays(K)
    r = normal_equation_residual(g.l_points(), arr[1], arr[2], arr[3], arr[4], g.deltas(), 1e-4)
    return {"rel_max": r["rel_max"], "rel_l2": r["rel_l2"], "max_abs_residual": r["max_abs_res"], "max_abs_rhs": r["max_abs_rhs"],
            "what": "max |(J'WJ + lambda I) dx - J'W r| / max_i sum_f |J_f'W_f r_f|_i of the last resident iteration, matrix-free in numpy"}


def lattice1m(lib, rank, world, device, backend, barrier, sync_all, K=1000, iters=2):
    """config 5.  world == 1: resident single-GPU iterations.  world > 1: one solve sharded over all ranks."""
    import torch
    t0 = time.perf_counter()
    g = lib.new_graph(); nfac = lib.dll.aprilsam_amd_make_lattice(g.ptr, K); p = lib.new_param()
    res = {"workload": f"synthetic {K}x{K} Manhattan lattice, {K * K} poses / {nfac} factors (config 5)", "n_gpus": world}
    lib.dll.aprilsam_amd_resident_chi2.restype = C.c_double
    if world == 1:
        assert lib.dll.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
        res["setup_s_incl_ordering_symbolic_upload"] = time.perf_counter() - t0
        chi = [lib.dll.aprilsam_amd_resident_chi2(g.ptr)]
        lib.dll.aprilsam_amd_resident_steps(g.ptr, p.ptr, 1, 0); assert lib.dll.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
        chi.append(lib.dll.aprilsam_amd_resident_chi2(g.ptr))
        dt = timed_steps(lib, g, p, iters, sync_all, barrier)
        chi.append(lib.dll.aprilsam_amd_resident_chi2(g.ptr))
        lib.dll.aprilsam_amd_resident_steps(g.ptr, p.ptr, 2, 1)
        lp = kernel_profile(lib, p); st = p.stats()
        levels = level_profile(lib, p, 2)
        fac_ms = sum(k["ms"] / 2 for k in lp if k["name"] in FACTOR_KERNELS)
        lev_ms = sum(L["factor_ms"] + L["backsolve_ms"] for L in levels)
        all_ms = sum(k["ms"] / 2 for k in lp)
        res["level_times"] = [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in L.items()} for L in levels]
        res["modelled_scaling_from_level_times"] = modelled_scaling_from_level_times(levels, max(all_ms - lev_ms, 0.0), all_ms)
        res.update(parallelism="single GPU", kernels_ms_per_step={k["name"]: round(k["ms"] / 2, 3) for k in lp},
                   nnz_L=st["nnz_L"], sum_cj2=st["flops_factor"], fronts=st["n_fronts"], levels=st["n_levels"],
                   max_front_rows=st["max_front_rows"], factor_tflops=st["flops_factor"] / (1e-3 * fac_ms) / 1e12,
                   roofline=big_front_rooflines(lp, 2, PMC_TAG + "_pmc_mfma_lattice1m.json"),
                   roofline_hbm=hbm_rooflines(lp, 2, PMC_TAG + "_pmc_hbm_lattice1m.json", survey_assembly_bytes(K * K, nfac - 1, 1)))
        lib.dll.aprilsam_amd_resident_end(g.ptr, p.ptr)
        try:
            res["normal_eq"] = normal_eq_check(lib, g, K); res["normal_eq_relres"] = res["normal_eq"]["rel_max"]
        except Exception as e:
            res["normal_eq"] = {"error": repr(e)}
    else:
        from aprilsam_amd.shard import ShardedSolver
        sol = ShardedSolver(lib, g, p, rank, world, backend=backend, device=device if backend == "nccl" else None)
        res["setup_s_incl_ordering_symbolic_upload"] = time.perf_counter() - t0
        chi = [sol.chi2()]
        sol.iterate(1)                                  # first iteration: also opens the point-to-point channels
        chi.append(sol.chi2())
        # parity that needs no recorded trace (normal_eq_check above): the first iteration's dx = gathered states - initial states against the
        # reference's normal equations at the initial states.  The gather is a collective of the library (every rank takes part); the numpy
        # part runs on rank 0, outside the timed region
        st1 = sol.gather_states()
        if rank == 0:
            try:
                from tests.support.normal_eq import normal_equation_residual
                arr = lib.lattice_arrays(K)
                dx1 = st1 - arr[0]
                dx1[:, 2] = (dx1[:, 2] + np.pi) % (2 * np.pi) - np.pi
                r = normal_equation_residual(arr[0], arr[1], arr[2], arr[3], arr[4], dx1, 1e-4)
                res["normal_eq"] = {"rel_max": r["rel_max"], "rel_l2": r["rel_l2"], "what": "first sharded iteration: dx = gathered states - initial states"}
                res["normal_eq_relres"] = r["rel_max"]
            except Exception as e:
                res["normal_eq"] = {"error": repr(e)}
        barrier(); torch.cuda.synchronize()
        t1 = time.perf_counter()
        sol.iterate(iters)                              # one library call: kernels and exchange on the solver stream
        torch.cuda.synchronize(); barrier()
        dt = sync_all(time.perf_counter() - t1)
        chi.append(sol.chi2())
        owned = int((sol.owner == rank).sum())
        res["comm"] = sol.comm_info()
        res["modelled_critical_path"] = sol.modelled_speedup()
        res.update(parallelism=f"nested-dissection subtree shards x{world}, exchange inside the library ({'RCCL on the solver stream' if backend == 'nccl' else 'host callbacks over ' + backend})",
                   fronts=int(sol.n_fronts), fronts_owned_by_rank0=owned, schur_slabs_exchanged=int(len(sol.xfer)),
                   separator_broadcasts=int(len(sol.bcast)), comm_bytes_per_iteration=sol.comm_bytes_per_iteration(),
                   front_pool_gb_rank0=8e-9 * sol.pool_doubles, front_pool_gb_whole_plan=8e-9 * sol.pool_doubles_all)
        sol.close()
    res.update(ms_per_step=1e3 * dt / iters, timed_iterations=iters, chi2=chi)
    if K == 1000 and iters == 2:
        res["chi2_relerr_vs_single_gpu"] = [abs(a - b) / b for a, b in zip(chi, LATTICE1M_CHI2)]
    if K == 316:      # config 4's lattice: the reference's own chi^2 before and after one iteration
        res["chi2_relerr_vs_reference"] = [abs(a - b) / b for a, b in zip(chi, LATTICE100K_CHI2)]
    p.destroy(); g.destroy()
    return res


MAX_LINE_BYTES = 8192       # the driver parses the LAST stdout line; round 5's 25.7 KB line came back as parsed = null
MAX_CONFIG_KEYS = 50


def sig(v, n=6):
    """floats to n significant digits (the line is read by a parser with a size limit: 17-digit floats are a third of its bytes)"""
    if isinstance(v, bool) or not isinstance(v, float):
        return v
    if v != v or v in (float("inf"), float("-inf")):
        return None
    return float(f"{v:.{n}g}")


def short_line(out):
    """The ONE stdout line: the contract fields, a FLAT `config` (scalars only, at most MAX_CONFIG_KEYS), a flat `roofline` (the dominant
    kernel's dict + per-kernel `_frac` / `_traffic_over_algorithmic` of the lattices) and `cpu_baseline`.  Everything nested -- per-level
    times, per-kernel roofline dicts, API split, incremental histogram, modelled scaling -- goes to the side file (write_extras)."""
    def scalar(v):
        return v is None or isinstance(v, (bool, int, float, str))
    cfg = {}
    roof = {}

    def put(dst, key, v):
        if isinstance(v, (list, tuple)) and all(scalar(x) for x in v):          # short vectors: one key per element
            for i, x in enumerate(v):
                dst[f"{key}_{i}"] = sig(x)
        elif scalar(v):
            dst[key] = sig(v)
    base = out["config"]
    for k in ("workload", "parallelism", "fronts", "levels", "nnz_L", "sum_cj2"):
        put(cfg, k, base.get(k))
    # ---- SURVEY 8(d)'s metric: one warm april_graph_cholesky call through the C-ABI -------------------------------------------------
    put(cfg, "api_call_it_per_s", out.get("value_api_call")); put(cfg, "ms_per_api_call", out.get("ms_per_api_call"))
    api = out.get("api", {})
    if "default" in api:
        put(cfg, "api_call_cold_ms", api.get("cold_ms_per_call"))
    if "error" in api:
        put(cfg, "api_error", api["error"])
    if "cpu_baseline" in out:
        put(cfg, "api_call_speedup_vs_reference_cpu", out.get("speedup_vs_cpu_baseline"))
        put(cfg, "resident_speedup_vs_reference_cpu", out.get("speedup_resident_vs_cpu_baseline"))
        put(cfg, "cold_call_speedup_vs_reference_cpu", out.get("speedup_vs_cpu_baseline_cold_call"))
    put(cfg, "parity_chi2_max_relerr_10_iters", out.get("parity", {}).get("chi2_max_relerr_10_iters"))
    put(cfg, "parity_max_abs_state_err", out.get("parity", {}).get("max_abs_state_err"))
    # ---- config 4 -------------------------------------------------------------------------------------------------------------------
    l100 = out.get("lattice100k", {})
    for k in ("ms_per_step", "speedup_vs_reference_cpu", "chi2_relerr_vs_reference", "normal_eq_relres", "factor_tflops", "error"):
        if k in l100:
            put(cfg, f"lattice100k_{k}", l100[k])
    rc = l100.get("reference_cpu_same_host")
    if isinstance(rc, dict):
        put(cfg, "lattice100k_reference_cpu_s_per_iter", rc.get("s_per_iter"))
    # ---- config 5 -------------------------------------------------------------------------------------------------------------------
    l1m = out.get("lattice1m", {})
    for k in ("ms_per_step", "n_gpus", "factor_tflops", "normal_eq_relres", "comm_bytes_per_iteration", "error"):
        if k in l1m:
            put(cfg, f"lattice1m_{k}", l1m[k])
    for k in ("chi2_relerr_vs_single_gpu", "chi2_relerr_vs_reference"):      # (K = 1000: the recorded single-GPU trace; K = 316: the reference's own chi^2)
        if isinstance(l1m.get(k), list) and l1m[k]:
            put(cfg, "lattice1m_chi2_relerr_max", max(l1m[k]))
    if isinstance(l1m.get("comm"), dict):
        for k in ("transport", "ncclCommCount"):
            if k in l1m["comm"]:
                put(cfg, f"lattice1m_{k}", l1m["comm"][k])
    msc = l1m.get("modelled_scaling_from_level_times")
    if isinstance(msc, dict) and isinstance(msc.get("G8"), dict):
        put(cfg, "lattice1m_modelled_G8_speedup_owner", msc["G8"].get("speedup_top_fronts_on_one_owner"))
    # ---- config 3 and the growing-graph batch mode ----------------------------------------------------------------------------------
    inc = out.get("m3500_incremental", {})
    for k, name in (("total_ms", "inc_total_ms"), ("median_ms", "inc_median_ms"), ("speedup_total_vs_reference", "inc_speedup_vs_reference"),
                    ("fallback_schedule_identical", "inc_fallbacks_identical"), ("chi2_max_relerr_vs_reference", "inc_chi2_max_relerr_vs_reference"), ("error", "inc_error")):
        if k in inc:
            put(cfg, name, inc[k])
    gb = out.get("m3500_batch_update_only", {})
    for k, name in (("speedup_total_vs_reference", "batch_only_speedup"), ("total_ms", "batch_only_total_ms"), ("error", "batch_only_error")):
        if k in gb:
            put(cfg, name, gb[k])
    # ---- per-kernel ms per iteration (kernels that ran) -----------------------------------------------------------------------------
    for tag, blk in (("m3500", out), ("l100k", l100), ("l1m", l1m)):
        for k, v in (blk.get("kernels_ms_per_step") or {}).items():
            if v:
                put(cfg, f"{tag}_ms_{k}", float(v))
    if len(cfg) > MAX_CONFIG_KEYS:          # (never the headline keys above: the per-kernel ms of the lattices go first)
        for k in [k for k in list(cfg)[::-1] if "_ms_k_" in k][:len(cfg) - MAX_CONFIG_KEYS]:
            del cfg[k]
    # ---- roofline: the dominant kernel of `value`'s workload, then fractions of the lattices' kernels -------------------------------
    for k, v in out.get("roofline", {}).items():
        if scalar(v):
            roof[k] = sig(v)
    for tag, blk in (("l100k", l100), ("l1m", l1m)):
        for r in (blk.get("roofline") or []) + (blk.get("roofline_hbm") or []):
            kn = r.get("kernel")
            if kn == "k_front_small" and r.get("bound") == "hbm":
                kn = "k_front_small_hbm"
            for k in ("frac", "traffic_over_algorithmic"):
                if k in r and scalar(r[k]):
                    roof[f"{tag}_{kn}_{k}"] = sig(r[k], 4)
    line = {k: sig(out.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                                         "dtype", "data")}
    line["config"] = cfg
    if roof:                                # (a plain run has no instrumented pass)
        line["roofline"] = roof
    if "cpu_baseline" in out:
        line["cpu_baseline"] = {k: sig(v) for k, v in out["cpu_baseline"].items() if scalar(v)}
    for k in ("factorise_ms", "value_api_call", "ms_per_api_call", "source_hash", "value_definition", "vs_baseline_definition", "extras"):
        if k in out:
            line[k] = sig(out[k])
    return line


def write_extras(out):
    """the full nested record: bench_extras.json (next to gpurun_out/ when it exists: that directory travels back from the GPU box) + stderr"""
    d = os.path.join(ROOT, "gpurun_out")
    path = os.path.join(d if os.path.isdir(d) else ROOT, "bench_extras.json")
    try:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        out["extras"] = os.path.relpath(path, ROOT)
    except OSError as e:
        out["extras"] = f"not written: {e}"
    print("bench extras: " + json.dumps(out), file=sys.stderr, flush=True)


def emit(out, full=True):
    if full:
        write_extras(out)
    s = json.dumps(short_line(out))
    assert len(s.encode()) < MAX_LINE_BYTES, f"bench line is {len(s.encode())} bytes"
    print(s, flush=True)


MAX_DUMP_BYTES = 64 << 20


def dump_outputs(d, arrays):
    """--dump-outputs: what the timed path hands its caller after its last step, as <d>/<name>.npy (float64) -- for comparing two builds
    output for output (the inputs are the committed M3500 fixture, so they are the same in every run)"""
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    assert sum(v.nbytes for v in arrays.values()) <= MAX_DUMP_BYTES
    os.makedirs(d, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(d, k + ".npy"), v)


def aggregate_value(world, steps, max_dt):
    """whole-job throughput of `world` independent replicas: GN iterations / s"""
    return world * steps / max_dt


def full_record(a, lib, arrays, out, rank, world, local, device, barrier, sync_all):
    """--full: everything beyond the headline figure, added to `out`.  Every rank takes part (the API calls and config 5 are timed
    between barriers)."""
    import torch
    from aprilsam_amd import datasets, host
    # ---- parity gate on this very build: 10 iterations vs the reference golden -----------------------------
    G = np.load(os.path.join(ROOT, "tests", "golden", "m3500_batch.npz"))
    g = lib.new_graph(); g.build_from_arrays(*arrays); p = lib.new_param()
    chi2, _ = g.batch_resident(p, 10)
    chi2_err = float(np.max(np.abs(chi2 - G["chi2"]) / G["chi2"]))
    state_err = float(np.max(np.abs(g.states() - G["final_states"])))
    p.destroy(); g.destroy()
    assert chi2_err < 1e-6, f"parity gate failed: chi2 relative error {chi2_err}"

    # ---- instrumented pass: K steps of a second resident copy after the same warm-up, every kernel launch timed with HIP events on the
    #      solver stream ------------------------------------------------------------------------------------------------------
    g = lib.new_graph(); g.build_from_arrays(*arrays); p = lib.new_param()
    assert lib.dll.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    lib.dll.aprilsam_amd_resident_steps(g.ptr, p.ptr, a.warmup, 0)
    lib.dll.aprilsam_amd_resident_sync(g.ptr, p.ptr)
    lib.dll.aprilsam_amd_resident_steps(g.ptr, p.ptr, a.steps, 1)
    prof = kernel_profile(lib, p)
    lib.dll.aprilsam_amd_resident_end(g.ptr, p.ptr)
    p.destroy(); g.destroy()

    # ---- the same K steps as K warm april_graph_cholesky calls through the C-ABI (SURVEY.md section 8(d)'s metric): host
    #      objects in, states valid in the host objects on return, every call synchronises itself --------------------------
    g = lib.new_graph(); g.build_from_arrays(*arrays); p = lib.new_param()
    for _ in range(max(a.warmup, 3)):
        g.cholesky(p)
    barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        g.cholesky(p)
    torch.cuda.synchronize(); barrier()
    dt_api = sync_all(time.perf_counter() - t0)
    assert p.stats()["not_spd"] == 0 and p.stats()["error_code"] == 0
    p.destroy(); g.destroy()
    for k in prof:
        k["ms_per_iter"] = k["ms"] / a.steps; k["launches_per_iter"] = k["calls"] / a.steps
    dom = max(prof, key=lambda k: k["ms"])
    dur_s = dom["ms_per_iter"] * 1e-3
    if dom["name"] in FLOP_KERNELS:
        ach = dom["flops"] / dur_s / 1e12
        roof = dict(bound="mfma", achieved=ach, peak=FP64_PEAK_TFLOPS, unit="TFLOP/s", frac=ach / FP64_PEAK_TFLOPS)
    else:
        ach = dom["bytes"] / dur_s / 1e9
        roof = dict(bound="hbm", achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach / HBM_PEAK_GBS)
    # HBM traffic of that kernel per launch from the committed PMC passes (profiles/, separate rocprofv3 --pmc runs of
    # this same workload): (2 x FETCH_SIZE + WRITE_SIZE) KB — the x2 on the read side is the gfx950 correction of
    # MI355X_MICROARCH.md section HBM (calibrated there for wide coalesced reads; our 8-byte loads are uncalibrated)
    traffic = None
    pmc, pmc_src = load_pmc(PMC_TAG + "_pmc_hbm.json")
    try:
        cn = pmc["counters"]
        traffic = 1024.0 * (2.0 * cn["FETCH_SIZE"][dom["name"]]["kb_per_dispatch"] + cn["WRITE_SIZE"][dom["name"]]["kb_per_dispatch"])
    except Exception:
        pass
    if traffic and dom["bytes"] > 0:        # HBM bytes the counters saw per iteration over the kernel's algorithmic bytes (SURVEY 8(d) conventions)
        roof["traffic_per_step"] = traffic * dom["launches_per_iter"]
        roof["traffic_over_algorithmic"] = roof["traffic_per_step"] / dom["bytes"]
        roof["algorithmic_bytes_per_step"] = dom["bytes"]
    roof.update(kernel=dom["name"], traffic=traffic, traffic_source=(pmc_src + " (bytes per launch)") if traffic else pmc_src,
                avg_launch_us=1e3 * dom["ms"] / max(1, dom["calls"]),
                launches_per_step=dom["launches_per_iter"], kernel_ms_per_step=dom["ms_per_iter"],
                algorithmic_work_per_step=dom["flops"] if dom["name"] in FLOP_KERNELS else dom["bytes"],
                measured="HIP events around every launch, instrumented pass of the same K steps")
    factorise_ms = sum(k["ms_per_iter"] for k in prof if k["name"] in FACTOR_KERNELS)

    out.update({
        "value_api_call": aggregate_value(world, a.steps, dt_api), "ms_per_api_call": 1e3 * dt_api / a.steps,
        "value_definition": "value = resident loop (inputs in HBM, bench contract); value_api_call = warm april_graph_cholesky calls through the C-ABI "
                            "(SURVEY 8(d)'s metric)",
        "factorise_ms": factorise_ms,
        "parity": {"chi2_max_relerr_10_iters": chi2_err, "max_abs_state_err": state_err, "bar": 1e-6},
        "roofline": roof,
        "kernels_ms_per_step": {k["name"]: round(k["ms_per_iter"], 5) for k in prof},
        "kernel_launches_per_step": {k["name"]: k["launches_per_iter"] for k in prof},
        "multi_gpu": {"world": world, "backend": a.backend, "rank0_device": local,
                      "transport": ("host callbacks over gloo (test mode)" if a.backend != "nccl" else "RCCL") if world > 1 else "none (single rank)",
                      "rccl_version_torch": ".".join(str(v) for v in torch.cuda.nccl.version()) if world > 1 and a.backend == "nccl" else None,
                      "data_path_collectives": "none for `value` (independent replicas); lattice1m: ncclSend/ncclRecv of Schur slabs + ncclBroadcast of separator solutions inside the library"},
    })
    if rank == 0 and world == 1 and not a.no_lattice:
        try:
            arr = lib.lattice_arrays(316)
            g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
            t0 = time.perf_counter()
            lib.dll.aprilsam_amd_resident_begin(g.ptr, p.ptr)
            sym_ms = (time.perf_counter() - t0) * 1e3
            c0 = lib.dll.aprilsam_amd_resident_chi2  # noqa
            lib.dll.aprilsam_amd_resident_chi2.restype = C.c_double
            chi0 = lib.dll.aprilsam_amd_resident_chi2(g.ptr)
            lib.dll.aprilsam_amd_resident_steps(g.ptr, p.ptr, 1, 0); lib.dll.aprilsam_amd_resident_sync(g.ptr, p.ptr)
            chi1 = lib.dll.aprilsam_amd_resident_chi2(g.ptr)
            ks = 10
            dtl = timed_steps(lib, g, p, ks, lambda x: x, lambda: None)
            lib.dll.aprilsam_amd_resident_steps(g.ptr, p.ptr, 3, 1)
            lp = kernel_profile(lib, p); ls = p.stats()
            lv100 = level_profile(lib, p, 3)
            out["lattice100k"] = {
                "level_times": [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in L.items()} for L in lv100],
                "workload": "synthetic 316x316 Manhattan lattice, 99856 poses / 397531 factors (config 4)",
                "ms_per_step": 1e3 * dtl / ks, "first_call_ms_incl_symbolic": sym_ms,
                "chi2_0": chi0, "chi2_after_1": chi1,
                "chi2_relerr_vs_reference": [abs(chi0 - LATTICE100K_CHI2[0]) / LATTICE100K_CHI2[0], abs(chi1 - LATTICE100K_CHI2[1]) / LATTICE100K_CHI2[1]],
                "reference_cpu_s_per_iter_survey_container": 44.8,
                "nnz_L": ls["nnz_L"], "sum_cj2": ls["flops_factor"], "fronts": ls["n_fronts"], "levels": ls["n_levels"],
                "kernels_ms_per_step": {k["name"]: round(k["ms"] / 3, 4) for k in lp},
                "factor_tflops": ls["flops_factor"] / (1e-3 * sum(k["ms"] / 3 for k in lp if k["name"] in FACTOR_KERNELS)) / 1e12,
                "roofline": big_front_rooflines(lp, 3, PMC_TAG + "_pmc_mfma.json"),
                "roofline_hbm": hbm_rooflines(lp, 3, PMC_TAG + "_pmc_hbm_lattice100k.json", survey_assembly_bytes(316 * 316, len(arr[1]) - 1, 1)),
            }
            lib.dll.aprilsam_amd_resident_end(g.ptr, p.ptr)
            try:
                out["lattice100k"]["normal_eq"] = normal_eq_check(lib, g, 316); out["lattice100k"]["normal_eq_relres"] = out["lattice100k"]["normal_eq"]["rel_max"]
            except Exception as e:
                out["lattice100k"]["normal_eq"] = {"error": repr(e)}
            p.destroy(); g.destroy()
            # the reference on the same lattice on THIS host: measured when asked for (--cpu-lattice100k, one call = one iteration,
            # about a minute), otherwise the figure recorded by such a run on the GPU box (profiles/, same hardware class)
            from tests.support.oracle_binding import REFLIB
            rec = os.path.join(ROOT, "profiles", PMC_TAG + "_cpu_lattice100k.json")
            if not (a.no_cpu_lattice100k or a.no_cpu_baseline) and os.path.exists(REFLIB):
                ref = host.SolverLib(REFLIB)
                g = ref.new_graph(); g.build_from_arrays(*arr); p = ref.new_param()
                t0 = time.perf_counter(); g.cholesky(p); cpu_s = time.perf_counter() - t0
                out["lattice100k"]["reference_cpu_same_host"] = {"s_per_iter": cpu_s, "cores": 1, "chi2_after_1": g.chi2(), "measured": "this run",
                                                                  "host": f"{os.cpu_count()} logical cores visible"}
                p.destroy(); g.destroy()
            elif os.path.exists(rec):
                out["lattice100k"]["reference_cpu_same_host"] = dict(json.load(open(rec)), measured="profiles/" + os.path.basename(rec))
            if "reference_cpu_same_host" in out["lattice100k"]:
                out["lattice100k"]["speedup_vs_reference_cpu"] = 1e3 * out["lattice100k"]["reference_cpu_same_host"]["s_per_iter"] / out["lattice100k"]["ms_per_step"]
        except Exception as e:   # the headline line must survive a failure of the extra
            out["lattice100k"] = {"error": repr(e)}
    if rank == 0 and world == 1 and not a.no_inc:
        # config 3: the pose-by-pose M3500 demo (examples/aprilsam_demo.c semantics, deterministic schedule)
        try:
            from aprilsam_amd import harness
            from tests.support.oracle_binding import REFLIB
            G = np.load(os.path.join(ROOT, "tests", "golden", "m3500_inc_demo.npz"))
            res = harness.run_demo(lib, datasets.m3500_arrays(), deterministic=True)
            ms = res["ms"]
            rel = np.abs(res["chi2"] - G["chi2"]) / np.maximum(G["chi2"], 1e-9)
            inc = {"workload": "M3500 demo, 3500 poses added one by one: 1 batch + 3499 april_graph_cholesky_inc calls through the "
                               "reference API (host objects in/out every call), nthreshold 100, delta 0.1/0.1, wall-clock rule off",
                   "total_ms": float(ms.sum()), "mean_ms": float(ms.mean()), "median_ms": float(np.median(ms)),
                   "p99_ms": float(np.percentile(ms, 99)), "max_ms": float(ms.max()),
                   "chi2_max_relerr_vs_reference": float(rel.max()), "final_chi2": float(res["chi2"][-1]),
                   "batch_fallbacks": int(res["was_batch"].sum()) - 1,
                   "fallback_schedule_identical": bool(np.array_equal(res["was_batch"], G["was_batch"])),
                   "max_abs_state_err": float(np.max(np.abs(res["final_states"] - G["final_states"])))}
            wb = res["was_batch"]; small = (~wb) & (ms <= 0.1)
            inc["where_the_time_goes"] = {   # steps with a batch fall-back inside / steps that stay in the last tail front (one launch) / loop closures
                "fallback_steps": int(wb.sum()), "fallback_ms": float(ms[wb].sum()),
                "steps_up_to_0.1_ms": int(small.sum()), "their_ms": float(ms[small].sum()),
                "steps_above_0.1_ms": int(((~wb) & ~small).sum()), "their_ms_": float(ms[(~wb) & ~small].sum())}
            if os.path.exists(REFLIB) and not a.no_cpu_baseline:
                ref = host.SolverLib(REFLIB)
                rr = harness.run_demo(ref, datasets.m3500_arrays(), deterministic=True)
                rms = rr["ms"]
                inc["reference_cpu_same_host"] = {"total_ms": float(rms.sum()), "mean_ms": float(rms.mean()), "median_ms": float(np.median(rms)),
                                                   "p99_ms": float(np.percentile(rms, 99)), "max_ms": float(rms.max()), "cores": 1}
                inc["speedup_total_vs_reference"] = float(rms.sum() / ms.sum())
            out["m3500_incremental"] = inc
        except Exception as e:
            out["m3500_incremental"] = {"error": repr(e)}
    if rank == 0 and world == 1:
        try:
            out["api"] = api_calls(lib, arrays)
        except Exception as e:
            out["api"] = {"error": repr(e)}
    if rank == 0 and world == 1 and not a.no_inc:
        # the cold call in its natural habitat: the reference demo's --batch_update_only mode (examples/aprilsam_demo.c:224-228),
        # one april_graph_cholesky per new pose on a growing graph -- every call sees a new topology
        try:
            from aprilsam_amd import harness
            from tests.support.oracle_binding import REFLIB
            npos = 1200
            r = harness.run_demo(lib, datasets.m3500_arrays(), batch_update_only=True, max_poses=npos)
            ms = r["ms"][1:]
            gb = {"workload": f"M3500 demo --batch_update_only, first {npos} poses: one april_graph_cholesky call per new pose through the reference API",
                  "total_ms": float(ms.sum()), "mean_ms": float(ms.mean()), "median_ms": float(np.median(ms)), "p99_ms": float(np.percentile(ms, 99)),
                  "final_chi2": float(r["chi2"][-1]),
                  "note": "batch_extend: the plan is kept while the graph only grows (appended poses become tail fronts, every front is "
                          "re-factorised); full re-plan every 3 x 24 appended poses (extend_tail_fronts)"}
            if os.path.exists(REFLIB) and not a.no_cpu_baseline:
                rr = harness.run_demo(host.SolverLib(REFLIB), datasets.m3500_arrays(), batch_update_only=True, max_poses=npos)
                rms = rr["ms"][1:]
                gb["reference_cpu_same_host"] = {"total_ms": float(rms.sum()), "mean_ms": float(rms.mean()), "median_ms": float(np.median(rms)), "cores": 1,
                                                 "final_chi2": float(rr["chi2"][-1])}
                gb["speedup_total_vs_reference"] = float(rms.sum() / ms.sum())
                gb["chi2_max_relerr_vs_reference"] = float(np.max(np.abs(r["chi2"] - rr["chi2"]) / np.maximum(rr["chi2"], 1e-9)))
            out["m3500_batch_update_only"] = gb
        except Exception as e:
            out["m3500_batch_update_only"] = {"error": repr(e)}
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(arrays)
        out["cpu_baseline"]["host"] = f"{os.cpu_count()} logical cores visible; reference is single-threaded"
        # like for like: the reference's number is one whole april_graph_cholesky call, so is ours (API, warm, default options)
        out["speedup_vs_cpu_baseline"] = out["value_api_call"] / out["cpu_baseline"]["value"]
        if "default" in out.get("api", {}):
            out["speedup_vs_cpu_baseline_cold_call"] = 1e3 / out["api"]["cold_ms_per_call"] / out["cpu_baseline"]["value"]
        out["speedup_resident_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
        # BASELINE.md publishes no number for this metric; the round-5 review asked for the like-for-like ratio here: one warm
        # april_graph_cholesky call of this library against one of the unmodified reference on this host (1 thread)
        out["vs_baseline"] = out["speedup_vs_cpu_baseline"]
        out["vs_baseline_definition"] = "value_api_call / cpu_baseline.value (same host, 1 thread); BASELINE.md publishes no number"
    if a.lattice1m_k > 0 and not a.no_lattice:
        # config 5.  Every rank takes part when world > 1; the headline line must survive a hang of the exchange, so a
        # watchdog prints it (rank 0) and ends the process if the extra does not come back in time.
        import threading

        def give_up():
            if rank == 0:
                out["lattice1m"] = {"error": "watchdog: sharded solve did not finish in 240 s", "n_gpus": world}
                emit(out)
            os._exit(0)
        dog = threading.Timer(240.0, give_up); dog.daemon = True; dog.start()
        try:
            out["lattice1m"] = lattice1m(lib, rank, world, device, a.backend, barrier, sync_all, K=a.lattice1m_k)
        except Exception as e:
            out["lattice1m"] = {"error": repr(e), "n_gpus": world}
        dog.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the states, l_points and deltas they left as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true", help="also run everything beyond the headline figure (parity gate, roofline, API calls, "
                                                        "CPU baseline, lattices, incremental demo, side file); the --no-* options below apply to it")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-lattice", action="store_true")
    ap.add_argument("--no-inc", action="store_true")
    ap.add_argument("--lattice1m-k", type=int, default=1000, help="side of the config-5 lattice (0 = skip)")
    ap.add_argument("--backend", default="nccl", help="nccl (= RCCL; the driver's multi-GPU runs) | gloo (functional test, host staging)")
    ap.add_argument("--one-gpu", action="store_true", help="test mode: every rank uses cuda:0")
    ap.add_argument("--cpu-lattice100k", action="store_true", help="(default since round 5; kept for old command lines)")
    ap.add_argument("--no-cpu-lattice100k", action="store_true",
                    help="do NOT time one april_graph_cholesky call of the reference on the 100k lattice on this host (about half a minute of "
                         "CPU, single thread); the figure recorded under profiles/ is quoted instead")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    import torch
    import __graft_entry__ as ge
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local = 0 if a.one_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    if rank == 0:
        ge.build()
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    barrier, sync_all = setup_dist(world, a.backend, device if a.backend == "nccl" else torch.device("cpu"))
    from aprilsam_amd import datasets, host
    lib = host.SolverLib()
    lib.dll.aprilsam_amd_set_device(local)
    arrays = datasets.m3500_batch()

    # ---- timed region ------------------------------------------------------------------------------------------
    g = lib.new_graph(); g.build_from_arrays(*arrays); p = lib.new_param()
    t0 = time.perf_counter()
    assert lib.dll.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    first_call_ms = (time.perf_counter() - t0) * 1e3            # pack + ordering + symbolic + upload
    lib.dll.aprilsam_amd_resident_steps(g.ptr, p.ptr, a.warmup, 0)
    lib.dll.aprilsam_amd_resident_sync(g.ptr, p.ptr)
    dt = timed_steps(lib, g, p, a.steps, sync_all, barrier)
    ms_per_step = 1e3 * dt / a.steps
    value = aggregate_value(world, a.steps, dt)

    stats = p.stats()
    # what the K steps hand the caller in the node objects: state, l_point (where the last step was linearised), delta_X (its dx)
    assert lib.dll.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, {"states": g.states(), "l_points": g.l_points(), "deltas": g.deltas()})
    p.destroy(); g.destroy()

    out = {
        "metric": "Gauss-Newton iterations/sec + factorise ms on M3500 (chi2 match <=1e-6)",
        "value": value, "unit": "GN iterations/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "M3500 (reference data file, committed as fixture); synthetic only in `lattice100k`",
        "config": {"workload": "M3500 batch april_graph_cholesky, 1 replica per GPU (3500 poses, 5454 factors, n=10500)",
                   "parallelism": f"replicas x{world}" if world > 1 else "single GPU",
                   "fronts": stats["n_fronts"], "levels": stats["n_levels"], "nnz_L": stats["nnz_L"],
                   "sum_cj2": stats["flops_factor"], "leaf_nodes": 16},
        "first_call_ms_incl_symbolic": first_call_ms,
        "source_hash": source_hash(),
    }
    if a.full:
        full_record(a, lib, arrays, out, rank, world, local, device, barrier, sync_all)
    if rank == 0:
        emit(out, full=a.full)
    if world > 1:
        import torch.distributed as dist
        try:
            dist.barrier(); dist.destroy_process_group()
        except Exception:
            pass


if __name__ == "__main__":
    main()
