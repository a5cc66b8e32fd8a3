#!/usr/bin/env python3
"""debug: the up-sweep's critical path on M3500 from the front stamps (needs APRILSAM_AMD_KPROF=1, set here): from the front that ends last down
the child that ends last, per front start / wait seen / assembly done / factor done / end and its last child's end, us from the first workgroup's
start; then how many level-1 and level-2 fronts are dispatched, or end their prelude, after their last child has ended.
usage: up_sweep_stamps.py PERSIST_UP [leaves]     PERSIST_UP: the option's value, -1 = leave it alone (another build through APRILSAM_AMD_LIB);
leaves: also the leaves' durations by own pose blocks"""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["APRILSAM_AMD_KPROF"] = "1"
from aprilsam_amd import datasets, host
from tests.support.mf_emulator import PlanView
lib = host.SolverLib()
v = int(sys.argv[1])
if v >= 0:
    lib.set_option("persist_up", v)
arr = datasets.m3500_batch()
g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
lib.set_option("use_graph", 0)
for _ in range(4):
    g.cholesky(p)
st = p.stats(); nF = st["n_fronts"]
buf = np.zeros((nF, 16), np.int64)
n = lib.dll.aprilsam_amd_debug_front_times(p.ptr, buf.ctypes.data_as(C.POINTER(C.c_longlong)), nF)
P = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], leaf_nodes=16)
lev = np.asarray(P.front_level)
t0 = buf[:, 0][buf[:, 0] > 0].min()
us = lambda x: (x - t0) * 0.01
kids = lambda t: list(P.ch_idx[P.ch_ptr[t]:P.ch_ptr[t + 1]])
leaves = [t for t in range(nF) if lev[t] == 0]
print(f"== persist_up {v}: up_launch_fronts {st.get('up_launch_fronts')} error {st['error_code']}; sweep {us(buf[:, 3].max()):.1f} us; leaves: start min {us(min(buf[t,0] for t in leaves)):.1f} max {us(max(buf[t,0] for t in leaves)):.1f}, end max {us(max(buf[t,3] for t in leaves)):.1f}; "
      f"store mean {np.mean([(buf[t,3]-buf[t,2])*0.01 for t in leaves]):.2f} max {max((buf[t,3]-buf[t,2])*0.01 for t in leaves):.2f}")
t = int(np.argmax(buf[:, 3]))
while True:
    ks = kids(t)
    lce = us(max(buf[c, 3] for c in ks)) if ks else float('nan')
    ws = us(buf[t, 11]) if buf[t, 11] else float('nan')
    print(f"  L{lev[t]} front {t}: start {us(buf[t,0]):7.1f} wait seen {ws:7.1f} asm done {us(buf[t,1]):7.1f} fac done {us(buf[t,2]):7.1f} end {us(buf[t,3]):7.1f} | last child end {lce:7.1f} | prelude zero {(buf[t,4]-buf[t,0])*0.01:.1f} dest {(buf[t,5]-buf[t,4])*0.01:.1f} fill {(buf[t,6]-buf[t,5])*0.01:.1f} | xcd {buf[t,12]-1}")
    if not ks:
        break
    t = int(max(ks, key=lambda c: buf[c, 3]))
for L in (1, 2):
    fr = [t for t in range(nF) if lev[t] == L]
    late = sum(1 for t in fr if buf[t, 0] > max(buf[c, 3] for c in kids(t)))
    latep = sum(1 for t in fr if buf[t, 6] > max(buf[c, 3] for c in kids(t)))
    s = np.array([us(buf[t, 0]) for t in fr])
    print(f"  level {L}: {len(fr)} fronts, {late} start after their last child has ended, {latep} end their prelude after it; start min {s.min():.1f} median {np.median(s):.1f} max {s.max():.1f}; end max {us(max(buf[t,3] for t in fr)):.1f}")
if len(sys.argv) > 2 and sys.argv[2] == "leaves":
    nsb = np.asarray(P.front_nsb)
    print("  leaves by own pose blocks: nsb: count, median / max duration us (start -> end)")
    for b in sorted(set(int(nsb[t]) for t in leaves)):
        d = np.array([(buf[t, 3] - buf[t, 0]) * 0.01 for t in leaves if nsb[t] == b])
        print(f"    nsb {b:3d}: {len(d):4d} fronts, {np.median(d):6.2f} / {d.max():6.2f}")
