"""Pose graphs whose multifrontal plan is DESIGNED, front by front: clique trees.  TEST-ONLY.

Every cluster of poses is a clique, every cluster is fully connected to all its ancestor clusters, cluster sizes do not increase
towards the root, poses are numbered leaves first.  The ordering then finds the clusters again: a cluster of `a` poses under ancestors
totalling `b` poses becomes ONE front with s = 3a own columns, u = 3b update rows and one child per child cluster
(tests/test_clique_tree_plans.py holds every case below to that, on the library's own plan).  What does NOT work is a child cluster
smaller than its parent: the ordering merges those ((10, 40, 50) collapses, as does (20, 20, 70)).

CASES puts fronts on both sides of every size at which build_level or a kernel changes form; CLASSES names those sizes from the
constants of kernels.hip.h, independently of the cases; tests/test_gpu_front_shapes.py runs every case on the GPU."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NOISE = np.array([0.3, 0.3, 0.1])
ANCHOR_W = np.diag([30.0, 30.0, 80.0])


def _constants():
    """the kernels' own tile / block sizes, read from the header that defines them"""
    text = open(os.path.join(ROOT, "aprilsam_amd", "csrc", "kernels.hip.h")).read()
    out = {}
    for name in ("TPB", "NB", "TILE", "OBP", "CAPQ", "BS_TALL_ROWS", "BSB_MAX_HELPERS", "BSB_MAXB"):
        m = re.search(r"\b%s = (\d+)\b" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    out["OBW"] = out["OBP"] * out["NB"]              # columns of an outer block
    out["BSB_FAR"] = out["BSB_MAXB"] * out["OBW"]
    return out


K = _constants()
R16 = 16                                             # columns of a register block of the elimination (factor_dense_blk)


def _sizes(level, n):
    """cluster sizes of one level: an int, or a tuple cycled over the level's n clusters"""
    if isinstance(level, (tuple, list)):
        return [int(level[i % len(level)]) for i in range(n)]
    return [int(level)] * n


def layout(levels, fan):
    """-> list of (first pose, size, depth from the leaves, parent cluster or -1), leaves first; cluster c of depth k has the
    children c * fan .. c * fan + fan - 1 of depth k - 1 (indices within their level)"""
    D = len(levels)
    counts = [fan ** (D - 1 - k) for k in range(D)]
    clusters, start, first = [], [], 0
    for k in range(D):
        start.append(len(clusters))
        for i, a in enumerate(_sizes(levels[k], counts[k])):
            clusters.append([first, a, k, -1]); first += a
    for k in range(D - 1):
        for i in range(counts[k]):
            clusters[start[k] + i][3] = start[k + 1] + i // fan
    return [tuple(c) for c in clusters]


def design(levels, fan):
    """the designed fronts: sorted list of (s, u, children), one per cluster"""
    cl = layout(levels, fan)
    out = []
    for (first, a, k, par) in cl:
        b, p = 0, par
        while p >= 0:
            b += cl[p][1]; p = cl[p][3]
        out.append((3 * a, 3 * b, fan if k > 0 else 0))
    return sorted(out)


def clique_tree(levels, fan, seed, anchored=True):
    """-> (states, fa, fb, z, W) as datasets.random_pose_graph gives them: seeded states (angles over the whole circle, positions along
    the tree, below), z = the true relative pose + noise (0.3, 0.3, 0.1), W full and SPD, both edge orientations.  anchored: one xytpos prior per pose near its state
    with W = diag(30, 30, 80) (fb = -1), which keeps the system well conditioned; unary factors do not change the plan."""
    rng = np.random.default_rng(seed)
    cl = layout(levels, fan)
    N = sum(c[1] for c in cl)
    # Positions follow the tree, because the solver hands them to the dissection as a hint (its median cut along the principal axis must
    # fall between clusters, not through one): leaf cluster i of n sits at i + 1/2 on a line, scaled to [-10, 10]; a parent sits between
    # its two middle children, so that half of its subtree lies on either side; poses scatter around their cluster's place by less than
    # the gap to the next one.  Angles are random over the whole circle.
    D, nleaf = len(levels), fan ** (len(levels) - 1)
    centre, idx = np.zeros(len(cl)), 0
    for k in range(D):
        span = fan ** k                                  # leaves under a cluster of depth k
        for i in range(fan ** (D - 1 - k)):
            centre[idx] = i + 0.5 if k == 0 else span * i + (span // fan) * (fan // 2)
            idx += 1
    cx = np.concatenate([np.full(c[1], centre[i]) for i, c in enumerate(cl)])
    states = np.column_stack([(cx + rng.uniform(-0.2, 0.2, N)) * (20.0 / nleaf) - 10.0, rng.uniform(-0.2, 0.2, N) * (20.0 / nleaf),
                              rng.uniform(-np.pi, np.pi, N)])
    ea, eb = [], []
    for (first, a, k, par) in cl:
        own = np.arange(first, first + a)
        i, j = np.triu_indices(a, 1)
        ea.append(own[i]); eb.append(own[j])
        p = par
        while p >= 0:
            anc = np.arange(cl[p][0], cl[p][0] + cl[p][1])
            ea.append(np.repeat(own, len(anc))); eb.append(np.tile(anc, a))
            p = cl[p][3]
    ea = np.concatenate(ea).astype(np.int64); eb = np.concatenate(eb).astype(np.int64)
    flip = rng.random(len(ea)) < 0.3
    fa, fb = np.where(flip, eb, ea), np.where(flip, ea, eb)
    E = len(fa)
    pa, pb = states[fa], states[fb]
    c, s = np.cos(pa[:, 2]), np.sin(pa[:, 2])
    dx, dy = pb[:, 0] - pa[:, 0], pb[:, 1] - pa[:, 1]
    z = np.column_stack([c * dx + s * dy, -s * dx + c * dy, pb[:, 2] - pa[:, 2]]) + rng.normal(size=(E, 3)) * NOISE
    M = rng.normal(size=(E, 3, 3))
    W = np.einsum("nij,nkj->nik", M, M) + np.diag([20.0, 20.0, 50.0])
    W = ((W + W.transpose(0, 2, 1)) / 2).reshape(E, 9)
    if anchored:
        ids = np.arange(N)
        fa = np.concatenate([fa, ids]); fb = np.concatenate([fb, np.full(N, -1)])
        z = np.vstack([z, states + rng.normal(size=(N, 3)) * NOISE])
        W = np.vstack([W, np.tile(ANCHOR_W.reshape(1, 9), (N, 1))])
    return states, fa.astype(np.int32), fb.astype(np.int32), np.ascontiguousarray(z), np.ascontiguousarray(W)


# ------------------------------------------------------------------------------------------------------
# shape classes, from the code's constants.  Per front: s own columns, u update rows (its update block has u + 1 rows with the
# right-hand side: what the parent's extend-add reads), ch children.  s and u are multiples of 3.
# ------------------------------------------------------------------------------------------------------
def _below(T):
    return lambda s, u, ch: (s < T) & (s >= T - 3)


def _above(T):
    return lambda s, u, ch: (s >= T) & (s < T + 3)


def bsb_blocks(s):
    return (s + K["OBW"] - 1) // K["OBW"]


CLASSES = {}
for _T, _what in ((R16, "one 16-column register block"), (K["NB"], "one 32-column panel"), (K["TILE"], "64 columns"),
                  (K["OBW"], "one outer block"), (2 * K["OBW"], "two outer blocks"), (K["BS_TALL_ROWS"], "BS_TALL_ROWS")):
    CLASSES[f"s last below {_T} ({_what})"] = _below(_T)
    CLASSES[f"s first at or above {_T} ({_what})"] = _above(_T)
CLASSES.update({
    "s exactly three 16-column blocks": lambda s, u, ch: s == 3 * R16,
    "s an exact multiple of 32, more than one panel": lambda s, u, ch: (s % K["NB"] == 0) & (s > K["NB"]) & (s < K["OBW"]),
    "s an exact multiple of 64, more than one": lambda s, u, ch: (s % K["TILE"] == 0) & (s > K["OBW"]) & (s % K["OBW"] != 0),
    "s exactly three or more outer blocks, no partial last block": lambda s, u, ch: (s % K["OBW"] == 0) & (s >= 3 * K["OBW"]),
    "u = 0": lambda s, u, ch: u == 0,
    "u + 1 < 64": lambda s, u, ch: (u > 0) & (u + 1 < 64),
    "u + 1 = 64: exactly one pass of the extend-add": lambda s, u, ch: u + 1 == 64,
    "64 < u + 1 <= 67: a second pass, nearly empty": lambda s, u, ch: (u + 1 > 64) & (u + 1 <= 67),
    "u + 1 last at or below 128: two passes, no rest()": lambda s, u, ch: (u + 1 <= 128) & (u + 1 > 125),
    "u + 1 first above 128: rest()": lambda s, u, ch: (u + 1 > 128) & (u + 1 <= 131),
    "128 < u <= TPB: the tallest block a granule hand-over takes": lambda s, u, ch: (u > 128) & (u <= K["TPB"]),
    "u > TPB: flag hand-over": lambda s, u, ch: u > K["TPB"],
    "no children": lambda s, u, ch: ch == 0,
    "0 < children < CAPQ": lambda s, u, ch: (ch > 0) & (ch < K["CAPQ"]),
    "children = CAPQ": lambda s, u, ch: ch == K["CAPQ"],
    "children = CAPQ + 1": lambda s, u, ch: ch == K["CAPQ"] + 1,
    "children > 2 CAPQ: two refills and more": lambda s, u, ch: ch > 2 * K["CAPQ"],
    "k_backsolve_blk: at most 2 blocks, no helper": lambda s, u, ch: (bsb_blocks(s) <= 2) & (s > K["OBW"]),
    "k_backsolve_blk: 3 to 7 blocks, 1 to 5 helpers": lambda s, u, ch: (bsb_blocks(s) >= 3) & (bsb_blocks(s) - 2 < K["BSB_MAX_HELPERS"]),
    "k_backsolve_blk: 8 blocks, every helper, no wrap": lambda s, u, ch: bsb_blocks(s) - 2 == K["BSB_MAX_HELPERS"],
    "k_backsolve_blk: 9 or more blocks, helpers wrap": lambda s, u, ch: bsb_blocks(s) - 2 > K["BSB_MAX_HELPERS"],
})
# ... and one class of a whole level: fronts wider than one outer block whose outer-block counts differ (the active() prefix of the
# outer-block launches shrinks from block to block)
LEVEL_CLASS = "a level with multi-workgroup fronts of unequal widths"


def level_has_unequal_big(s_of_level):
    nb = {int(bsb_blocks(s)) for s in s_of_level if s > K["OBW"]}
    return len(nb) >= 2


# ------------------------------------------------------------------------------------------------------
# the cases: name -> (levels, fan, designed fronts, what the case is there for)
# ------------------------------------------------------------------------------------------------------
def _case(levels, fan, why):
    return (tuple(levels), fan, design(levels, fan), why)


CASES = {}
# (44,43 has four children, not three: with three leaves of 44 poses the dissection's median cut takes three poses of one leaf into the
# separator -- (123, 138, 0) under a root of 138 -- whatever the sizes nearby; four leaves split cleanly)
_CLIQUE_WHY = {1: "s = 3: a single pose", 5: "s = 15 < 16", 6: "s = 18 > 16", 10: "s = 30 < 32", 11: "s = 33 > 32", 16: "s = 48 = 3 x 16",
               21: "s = 63 < 64", 22: "s = 66 > 64", 32: "s = 96 = 3 x 32", 42: "s = 126 < 128", 43: "s = 129 > 128", 64: "s = 192 = 3 x 64",
               85: "s = 255 < 256", 86: "s = 258 > 256", 128: "s = 384 = 3 x 128, no partial outer block", 129: "s = 387 = 3 x 128 + 3",
               255: "s = 765 < BS_TALL_ROWS", 256: "s = 768 = BS_TALL_ROWS", 341: "s = 1023: 8 blocks of k_backsolve_blk, 6 helpers",
               342: "s = 1026: 9 blocks, helpers wrap"}
for _n, _why in _CLIQUE_WHY.items():
    CASES[f"clique {_n}"] = _case((_n,), 1, _why)
for _lv, _fan, _why in (((6, 5), 2, "smallest two-level tree"), ((11, 10), 2, "u = 30"), ((22, 21), 2, "u + 1 = 64: exactly one pass"),
                        ((23, 22), 2, "u + 1 = 67: a second 64-row pass"), ((43, 42), 2, "u + 1 = 127: two passes, no rest()"),
                        ((43, 43), 2, "u + 1 = 130: rest()"), ((44, 43), 4, "four children, s and u over one outer block"),
                        ((86, 85), 2, "s and u on either side of two outer blocks"), ((130, 128), 2, "children into a root of exactly three outer blocks"),
                        ((6, 5), 64, "children = CAPQ"), ((6, 5), 65, "children = CAPQ + 1"), ((6, 5), 129, "two refills of the staged child records + 1"),
                        ((17, 16), 65, "CAPQ + 1 children into s = 48")):
    CASES[f"{_lv[0]},{_lv[1]} x{_fan}"] = _case(_lv, _fan, _why)
CASES["5 x4 deep, fan 4"] = _case((5,) * 4, 4, "many tiny fronts, four levels")
CASES["30,25,20 fan 2"] = _case((30, 25, 20), 2, "three levels of unequal clusters")
CASES["44,43,43 fan 2"] = _case((44, 43, 43), 2, "u = 258 on the leaves, 129 in the middle")
CASES["16 x6 deep"] = _case((16,) * 6, 2, "tallest update block 240 rows: granule hand-over")
CASES["16 x7 deep"] = _case((16,) * 7, 2, "tallest update block 288 rows in a batch plan: flag hand-over")
CASES["mixed leaves 200,130,64 under 64"] = _case(((200, 130, 64), 64), 3, "multi-workgroup fronts of unequal widths on one level")

# Largest deviation of the oracle's dx from itself over three seeded random elimination orders (Oracle.batch_step(order=...)), over every
# case of the table above, anchored, at max |dx| of 0.06 .. 0.4: measured by tests/test_clique_tree_plans.py (which prints the figure per
# case and holds every case to this bound) -- 4.33e-15, on "6,5 x129" -- rounded up to one digit.  Without the anchors the same graphs deviate
# by 6e-11 .. 2e-10 (measured on four of them), which is why the cases are anchored.
ORDER_DEV = 5e-15
SEED = 7
