"""debug: per-level phase breakdown of k_backsolve (sets APRILSAM_AMD_KPROF=2): python tools/backsolve_times.py [--lattice K]
(gather = x of the struct rows in LDS; first products = up to the first block's barrier; rest = the remaining blocks / the chain);
then the gather of every child split by whether it ran on its parent's XCD (stamp slot 13 = 1 + XCC id);
then the hand-over of x inside the multi-level launch, per level for the front that ends last: from the end of its parent's chain (slot 7)
to its own "parent seen" (slot 4), split at the parent's stamps "last x store issued" (14), "stores drained, barrier passed" (11) and
"flag store issued" (15).  APRILSAM_AMD_TAGGED_X selects the hand-over (option tagged_x): with granules (1) there is no flag, slot 4 is
taken when the lanes start polling their own granules and slots 14 / 15 when the granule stores are issued -- compare the hop, parent's
chain end to child's gather end (slot 5), which means the same in every form.  Level 0 is the NEXT launch (its hop holds a kernel boundary)
unless the plan took it into the multi-level launch (option persist_leaves, APRILSAM_AMD_PERSIST_LEAVES=0 / 1: stats dn_launch_fronts then
counts every front); the last line gives the sweep's tail, from the last level-1 front's chain end to the last leaf's."""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["APRILSAM_AMD_KPROF"] = "2"
from aprilsam_amd import datasets, host
from tests.support.mf_emulator import PlanView
lib = host.SolverLib()
arr = lib.lattice_arrays(int(sys.argv[sys.argv.index("--lattice") + 1])) if "--lattice" in sys.argv else datasets.m3500_batch()
g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
lib.set_option("use_graph", 0)
for _ in range(3): g.cholesky(p)
nF = p.stats()["n_fronts"]
dn_fronts = p.stats()["dn_launch_fronts"]
buf = np.zeros((nF, 16), np.int64)
lib.dll.aprilsam_amd_debug_front_times(p.ptr, buf.ctypes.data_as(C.POINTER(C.c_longlong)), nF)
P = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], leaf_nodes=16)
for l in range(P.nLevels - 1, -1, -1):
    fr = P.lev_fronts[P.lev_ptr[l]:P.lev_ptr[l + 1]]
    big = max(fr, key=lambda t: buf[t, 7] - buf[t, 4])
    b = buf[big] * 0.01
    span = (max(buf[t, 7] for t in fr) - min(buf[t, 4] for t in fr)) * 0.01
    print(f"level {l}: span {span:.1f} | slowest nsb={P.front_nsb[big]} nub={P.front_nub[big]}: gather {b[5]-b[4]:.2f} first products {b[6]-b[5]:.2f} rest {b[7]-b[6]:.2f} total {b[7]-b[4]:.2f}")
X = buf[:, 13]
if X.any():
    groups = {}
    for t in range(nF):
        p = P.front_parent[t]
        if p < 0 or not X[t] or not X[p]:
            continue
        key = ("level 0" if P.front_level[t] == 0 else "levels 1+", "same" if X[t] == X[p] else "cross")
        groups.setdefault(key, []).append((buf[t, 5] - buf[t, 4]) * 0.01)
    for key in sorted(groups):
        v = np.array(groups[key])
        print(f"gather, {key[0]:9s} parent's XCD {key[1]:5s} n={len(v):3d}  mean {v.mean():5.2f} us  median {np.median(v):5.2f} us")
lv = {}
for t in range(nF):
    q = P.front_parent[t]
    if q >= 0 and buf[t, 4] and buf[q, 15]:
        lv.setdefault(P.front_level[t], []).append(t)
if lv:
    print(f"hand-over of x (tagged_x = {lib.get_option('tagged_x')}), us; per level the front that ends last, and the median over the level's fronts")
    print("level fronts |   hand-over = x stores + drain,barrier + write-back + flag-to-seen | gather |  hop (parent's chain end -> gather end) | median hop")
    tot = np.zeros(7)
    for l in sorted(lv, reverse=True):
        t = max(lv[l], key=lambda t: buf[t, 7]); q = P.front_parent[t]
        c, a = buf[t] * 0.01, buf[q] * 0.01
        row = np.array([c[4] - a[7], a[14] - a[7], a[11] - a[14], a[15] - a[11], c[4] - a[15], c[5] - c[4], c[5] - a[7]])
        if lib.get_option('tagged_x') == 1: row[[0, 2, 3, 4, 5]] = np.nan           # granules: no drain, no barrier, no flag -- slot 4 is not "parent seen", only the hop compares
        med = np.median([(buf[u, 5] - buf[P.front_parent[u], 7]) * 0.01 for u in lv[l]])
        tot += np.nan_to_num(row)
        print(f"{l:5d} {len(lv[l]):6d} | {row[0]:6.2f} = {row[1]:5.2f} + {row[2]:5.2f} + {row[3]:5.2f} + {row[4]:5.2f} | {row[5]:5.2f} | {row[6]:6.2f} | {med:6.2f}")
    n = len(lv)
    print(f" mean        | {tot[0]/n:6.2f} = {tot[1]/n:5.2f} + {tot[2]/n:5.2f} + {tot[3]/n:5.2f} + {tot[4]/n:5.2f} | {tot[5]/n:5.2f} | {tot[6]/n:6.2f} |   sum of hops {tot[6]:.2f}")
    if 0 in lv and 1 in lv:
        tail = (max(buf[t, 7] for t in lv[0]) - max(buf[t, 7] for t in lv[1])) * 0.01
        print(f"level 0 runs {'inside the multi-level launch' if dn_fronts == nF else 'as the NEXT launch'} ({dn_fronts} fronts in the launch): last leaf's chain end {tail:.2f} us after the last level-1 front's")
