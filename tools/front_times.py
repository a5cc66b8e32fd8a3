#!/usr/bin/env python3
"""debug: per-level phase breakdown of k_front_small (needs APRILSAM_AMD_KPROF=1); then the after-wait extend-add of every parent split by
whether its children ran on its XCD (stamp slot 12 = 1 + XCC id), and the XCD of each hop of the stamped critical path.
APRILSAM_AMD_XCD_PLACE=0 / 1 compares the level-by-level lists with the XCD-placed ones.
--process: instead, the stamps inside the extend-add behind the wait for the fronts of the critical path (see process_stamps).  These stamps
are compiled out of the product; --process --build-stamps first builds a library with them (build/ea_stamps/, a few minutes of hipcc, kept
until a source changes) and loads that one."""
import ctypes as C, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["APRILSAM_AMD_KPROF"] = "1"


def build_stamps_lib():
    """the product's sources and flags (__graft_entry__.build) plus -DAPRILSAM_AMD_EA_STAMPS -> build/ea_stamps/libaprilsam_amd.so"""
    import __graft_entry__ as G
    out = os.path.join(ROOT, "build", "ea_stamps", "libaprilsam_amd.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if G._newer(out, [os.path.join(G.CSRC, f) for f in G.SOURCES + G.HEADERS]):
        subprocess.check_call([G.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-DAPRILSAM_AMD_EA_STAMPS",
                               "-shared"] + [os.path.join(G.CSRC, s) for s in G.SOURCES] + ["-o", out], cwd=ROOT)
    return out


if "--build-stamps" in sys.argv:
    os.environ["APRILSAM_AMD_LIB"] = build_stamps_lib()      # (read when aprilsam_amd.host is imported: just below)
from aprilsam_amd import datasets, host
from tests.support.mf_emulator import PlanView
lib = host.SolverLib()


def process_stamps():
    """--process: the extend-add behind the wait (kernels.hip.h: PROF_EA_*), us after "wait passed", for the fronts of the up-sweep's critical path
    (from the front that ends last down the child that ends last): wave 0 (APRILSAM_AMD_KPROF=4), then per stamp the last wave to get there (5).
    Needs a library whose solver.hip.cpp was compiled with -DAPRILSAM_AMD_EA_STAMPS: --build-stamps makes and loads one (or load your own through
    APRILSAM_AMD_LIB).  The product is built without these stamps; with it this stops and says so."""
    arr = datasets.m3500_batch()
    lib.set_option("use_graph", 0)
    P = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], leaf_nodes=16)
    for mode, who in ((4, "wave 0"), (5, "last wave")):
        os.environ["APRILSAM_AMD_KPROF"] = str(mode)
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        for _ in range(4):
            g.cholesky(p)
        nF = p.stats()["n_fronts"]
        buf = np.zeros((nF, 16), np.int64)
        lib.dll.aprilsam_amd_debug_front_times(p.ptr, buf.ctypes.data_as(C.POINTER(C.c_longlong)), nF)
        # fronts waited for their children and none left a "rest done" stamp: slot 14 is the one of PROF_EA_* that nothing else writes in a
        # factorisation (without the stamps the pivot chain keeps its own figures in 8-10 and 15, which would be printed as if they were times)
        if buf[:, 11].any() and not buf[:, 14].any():
            sys.exit(f"front_times.py --process: the library loaded ({host.PRODUCT_LIB}) was compiled without -DAPRILSAM_AMD_EA_STAMPS, so the extend-add left no "
                     "stamps.  Run with --process --build-stamps, or point APRILSAM_AMD_LIB at a library built with that flag.")
        t0 = buf[:, 0][buf[:, 0] > 0].min()
        print(f"== {who}: sweep {(buf[:, 3].max() - t0) * 0.01:.1f} us; front (level, items of wave 0): loads issued / data back / adds done / rest done / last trip done / asm done, us after the wait")
        t, total = int(np.argmax(buf[:, 3])), 0.0
        while True:
            ks = list(P.ch_idx[P.ch_ptr[t]:P.ch_ptr[t + 1]])
            if not ks:
                break
            if buf[t, 11]:
                d = [(buf[t, k] - buf[t, 11]) * 0.01 if buf[t, k] else float("nan") for k in (8, 9, 10, 14, 15, 1)]
                total += d[5]
                print(f"  front {t:4d} (L{P.front_level[t]}, n={buf[t, 7]:2d}): " + " / ".join(f"{x:5.2f}" for x in d))
            t = int(max(ks, key=lambda c: buf[c, 3]))
        print(f"  after the wait, summed over the path: {total:.1f} us")
        p.destroy(); g.destroy()


if "--process" in sys.argv:
    process_stamps()
    sys.exit(0)
arr = datasets.m3500_batch() if "--lattice" not in sys.argv else lib.lattice_arrays(316)
g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
lib.set_option("use_graph", 0)
for _ in range(3):
    g.cholesky(p)
st = p.stats(); nF = st["n_fronts"]
buf = np.zeros((nF, 16), np.int64)
n = lib.dll.aprilsam_amd_debug_front_times(p.ptr, buf.ctypes.data_as(C.POINTER(C.c_longlong)), nF)
print("fronts", n)
perm = np.array([p.c.ordering[i] for i in range(len(arr[0]))])
P = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], leaf_nodes=16)
T = buf[:, :4] * 0.01   # us
for l in range(P.nLevels):
    fr = P.lev_fronts[P.lev_ptr[l]:P.lev_ptr[l + 1]]
    fr = [t for t in fr if T[t, 0] > 0]
    if not fr:
        print(f"level {l}: no small fronts"); continue
    a = np.array([[T[t, 1] - T[t, 0], T[t, 2] - T[t, 1], T[t, 3] - T[t, 2]] for t in fr])
    span = max(T[t, 3] for t in fr) - min(T[t, 0] for t in fr)
    big = max(fr, key=lambda t: T[t, 3] - T[t, 0])
    print(f"level {l}: {len(fr):4d} fronts  span {span:7.1f} us | mean asm {a[:,0].mean():6.1f} fac {a[:,1].mean():6.1f} store {a[:,2].mean():6.1f} | "
          f"slowest nsb={P.front_nsb[big]} nub={P.front_nub[big]} nch={P.ch_ptr[big+1]-P.ch_ptr[big]}: asm {T[big,1]-T[big,0]:.1f} fac {T[big,2]-T[big,1]:.1f} store {T[big,3]-T[big,2]:.1f} | chain+far {buf[big,8]*0.01:.1f} next-block syrk {buf[big,9]*0.01:.1f} (pure look-ahead chains {buf[big,15]*0.01:.2f} us = {buf[big,10]} cycles) | asm: zero {(buf[big,4]-buf[big,0])*0.01:.1f} dest {(buf[big,5]-buf[big,4])*0.01:.1f} fill {(buf[big,6]-buf[big,5])*0.01:.1f} (n={buf[big,7]}) rest {(buf[big,1]-buf[big,6])*0.01:.1f} (after wait {(buf[big,1]-buf[big,11])*0.01 if buf[big,11] else 0:.1f})")

# XCD split: after-wait extend-add per parent (wait seen -> assembly done), by where its children ran (slot 12 = 1 + XCC id)
X = buf[:, 12]
if X.any():
    groups = {}
    for t in range(nF):
        if P.front_level[t] < 1 or not buf[t, 11] or not X[t]:
            continue
        kids = [c for c in P.ch_idx[P.ch_ptr[t]:P.ch_ptr[t + 1]] if X[c]]
        if not kids:
            continue
        last = max(kids, key=lambda c: buf[c, 3])              # the child the wait was for
        frac = sum(X[c] == X[t] for c in kids) / len(kids)
        key = ("level 1" if P.front_level[t] == 1 else "levels 2+", "all" if frac == 1 else ("none" if frac == 0 else "some"))
        groups.setdefault(key, []).append((buf[t, 1] - buf[t, 11]) * 0.01)
        groups.setdefault((key[0], "last child " + ("same" if X[last] == X[t] else "cross")), []).append((buf[t, 1] - buf[t, 11]) * 0.01)
    for key in sorted(groups):
        v = np.array(groups[key])
        print(f"after wait, {key[0]:9s} children on the parent's XCD: {key[1]:17s} n={len(v):3d}  mean {v.mean():5.2f} us  median {np.median(v):5.2f} us")
    # the stamped critical path: from the root, the child that finished last
    t = int(max(range(nF), key=lambda u: buf[u, 3]))
    hops = []
    while True:
        kids = [c for c in P.ch_idx[P.ch_ptr[t]:P.ch_ptr[t + 1]] if X[c]]
        if not kids:
            break
        c = int(max(kids, key=lambda u: buf[u, 3]))
        hops.append(f"L{P.front_level[t]}:{'same' if X[c] == X[t] else 'cross'}({(buf[t, 1] - buf[t, 11]) * 0.01:.1f})")
        t = c
    print("critical path (level: child's XCD vs parent's, after-wait us):", " ".join(hops))
