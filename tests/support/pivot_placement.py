"""Placing the first non-positive pivot of a batch step at a chosen scalar position.  TEST INFRASTRUCTURE (numpy, no device).

The dense normal matrix A0 = J'WJ + lambda I of a graph at its states (tests/support/normal_eq.py's Jacobians) is permuted into the
library's elimination order (PlanView of tests/support/mf_emulator.py: `pos`, `front_first`, `front_nsb`, `front_level`, for the
`leaf_nodes` of the option set under test).  The knob is ONE extra xytpos prior on pose k with z = the pose's state (residual 0: the
right-hand side does not change) and W zero except W[d, d] = -s:

    A = A0 - s e_p e_p',        p = 3 pos[k] + d.

With d_p the p-th pivot of A0 in that order (the square of the Cholesky factor's diagonal entry):

* s = (1 + delta) d_p makes pivot p the FIRST non-positive one, equal to -delta d_p; every earlier pivot is unchanged;
* with s* = 1 / (A0^-1)_pp (s* <= d_p, equal for the very last pivot), A is positive definite exactly when s < s*.

For a p that is not the first column of a leaf the DIAGONAL entry A_pp - s can stay positive while the pivot is negative -- it does
whenever elimination has taken more than delta / (1 + delta) of A_pp, as at the last pivot of every graph here (case()["diag"]): these
systems are "indefinite with a positive diagonal".  A test that writes a
negative number on the diagonal of a leaf (diag(-50, 10, 10) on every factor of a pose) never produces one: there the very first pivot
a kernel looks at is the bad one, and the checks inside a block of columns are not exercised.

Position classes -- defined by the kernels (kernels.hip.h), not by a workload.  c = column inside its front, ns = 3 nsb own columns.

  chain_block (single-workgroup fronts; first pivot of a 16-wide block at `dn = readlane(D[0], 0)`, the others inside the unrolled chain)
    leaf_c0        c = 0 of a front on level 0
    blk_first      c = 0 (mod 16), c > 0
    blk_last       c = 15 (mod 16)
    interior       1 <= c mod 16 <= 14, not the last column of its front
    partial_last   c = ns - 1 of a front with ns mod 16 != 0 (the partial block)
    middle_level   an interior column of a front on a level strictly between the leaves and the top
    root_last      the last pivot of the last front: the only position a system that is indefinite by a small margin ever shows

  k_block_chain (option small_lds_kb = 0, a front with ns > 128; 32-column panels of 128-column outer blocks, diag_chain32)
    big_ob0_p0_m0      outer block 0, panel 0, c mod 32 = 0           (c = 0)
    big_ob0_p3_m31     outer block 0, panel 3, c mod 32 = 31          (c = 127)
    big_ob1_p0_mid     a later outer block, panel 0, interior column  (c = 128 + 7)
    big_ob1_p3_m0      a later outer block, panel 3, c mod 32 = 0     (c = 128 + 96)
    big_partial_last   c = ns - 1 with ns mod 32 != 0

A missed negative pivot turns into NaN, which the first pivot of the next block (or of the parent front) catches: the checks inside a
block carry the report alone only in the last block of the last front -- root_last and big_partial_last when the big front is the root.
"""
import functools

import numpy as np

from aprilsam_amd import datasets
from tests.support.consumer_graphs import two_components
from tests.support.mf_emulator import PlanView
from tests.support.normal_eq import linearise

SMALL_CLASSES = ["leaf_c0", "blk_first", "blk_last", "interior", "partial_last", "middle_level", "root_last"]
BIG_CLASSES = ["big_ob0_p0_m0", "big_ob0_p3_m31", "big_ob1_p0_mid", "big_ob1_p3_m0", "big_partial_last"]
CLASSES = SMALL_CLASSES + BIG_CLASSES
PLANS = (4, 16, 40)          # leaf_nodes of the option sets of tests/test_gpu_not_spd.py
DELTA = 0.25
# Levenberg-Marquardt on the chain with the knob (tests/test_lm_model.py, tests/test_gpu_not_spd.py): (class, delta).  Chosen for their model
# traces over 16 iterations (N: rejected, pivot not positive; A: accepted; r: rejected by rho): NNNNAAAArAArrArr, NNNNNNNAAAAANNAr,
# NNNNNNANANNAANNA -- rejections in a row at the start and again after accepted steps have shrunk lambda; every decision at least 9.9e-5 of
# the diagonal away from a zero pivot, 6000 x the float64 pivot error of tests/test_pivot_placement.py
LM_CASES = [("root_last", 4.0), ("interior", 0.25), ("leaf_c0", 0.25)]
LM_ITERS = 16
# 1000 x the worst float64 pivot error measured against the longer LDL' (1.5e-11).  The model's margin (min |d_j| / A_jj) is taken in NODE
# order, the device eliminates in its plan's order: the SIGN of the smallest pivot is the same in both (Sylvester), the margin is not.  The
# cases above keep the model's margin 6000 x above this figure, which is the room left for the other order.
LM_MARGIN = 1.5e-8


def chain(n, seed=3):
    """odometry chain with a prior on its LAST pose (tests/test_gpu_parity.py's _chain)"""
    rng = np.random.default_rng(seed)
    st = np.column_stack([np.arange(n, dtype=float), rng.normal(0, .2, n), rng.normal(0, .05, n)])
    fa = np.arange(n - 1, dtype=np.int32); fb = fa + 1
    z = np.column_stack([np.ones(n - 1), np.zeros(n - 1), np.zeros(n - 1)])
    W = np.tile(np.diag([100.0, 100.0, 400.0]).reshape(9), (n - 1, 1))
    return datasets.with_prior(st, fa, fb, z, W, first=False)


@functools.lru_cache(maxsize=None)
def graph(name):
    """the smallest graphs that offer every class: a random graph whose root front has 255 own columns (its last block of 16 and its last panel of 32 are partial, and the last pivot is not their first column) beside a second front above 128, the two-component
    graph of the consumer tests, a chain of 90 poses (270 scalars: the one the longer reference runs on)"""
    if name == "random":
        return datasets.random_pose_graph(280, 420, 3)
    if name == "two_components":
        return two_components()[0]
    if name == "chain":
        return chain(90)
    raise KeyError(name)


GRAPHS = ("random", "two_components", "chain")


def dense_normal(arr, lam):
    """A0 [3N, 3N] = sum_f J_f' W_f J_f + lam I and b [3N] = sum_f J_f' W_f r_f at the graph's states, node order"""
    st, fa, fb, z, W = arr
    st = np.asarray(st, float); N = len(st)
    fa = np.asarray(fa, np.int64); fb = np.asarray(fb, np.int64)
    W = np.asarray(W, float).reshape(-1, 3, 3)
    Ja, Jb, r = linearise(st, fa, fb, z)
    A = np.zeros((3 * N, 3 * N)); b = np.zeros(3 * N)
    for f in range(len(fa)):
        a = int(fa[f]); sa = slice(3 * a, 3 * a + 3)
        JtW = Ja[f].T @ W[f]
        A[sa, sa] += JtW @ Ja[f]; b[sa] += JtW @ r[f]
        if fb[f] >= 0:
            c = int(fb[f]); sc = slice(3 * c, 3 * c + 3)
            KtW = Jb[f].T @ W[f]
            A[sa, sc] += JtW @ Jb[f]; A[sc, sa] += KtW @ Ja[f]; A[sc, sc] += KtW @ Jb[f]; b[sc] += KtW @ r[f]
    A = 0.5 * (A + A.T)
    A[np.diag_indices(3 * N)] += lam
    return A, b


def with_knob(arr, k, d, s):
    """arr + the prior on pose k with z = its state and W = -s e_d e_d'; the knob is the LAST factor"""
    st, fa, fb, z, W = arr
    Wk = np.zeros(9); Wk[4 * d] = -s
    return (np.asarray(st, float), np.append(fa, k).astype(np.int32), np.append(fb, -1).astype(np.int32),
            np.vstack([np.asarray(z, float).reshape(-1, 3), np.asarray(st, float)[k]]), np.vstack([np.asarray(W, float).reshape(-1, 9), Wk]))


def ldl_pivots(A, dtype=np.float64, stop_at_first=False):
    """pivots of the LDL' factorisation without pivoting, right-looking, in `dtype` (np.longdouble: the longer reference).  Runs through
    negative pivots; stops at an exact zero (the pivots behind it come back NaN) or, with stop_at_first, at the first non-positive one"""
    M = np.array(A, dtype=dtype)
    n = len(M)
    d = np.full(n, np.nan, dtype=dtype)
    for j in range(n):
        d[j] = M[j, j]
        if d[j] == 0 or (stop_at_first and not d[j] > 0):
            break
        if j + 1 < n:
            col = M[j + 1:, j].copy()
            M[j + 1:, j + 1:] -= np.outer(col / d[j], col)
    return d


def first_non_positive(d):
    bad = np.nonzero(~(np.asarray(d) > 0))[0]
    return int(bad[0]) if len(bad) else -1


class Placement:
    """one graph under one plan: A0 in elimination order, its pivots, and the class -> (front, column) table"""

    def __init__(self, lib, name, leaf_nodes, lam):
        self.name, self.leaf_nodes, self.lam = name, leaf_nodes, lam
        self.arr = graph(name)
        st, fa, fb = self.arr[0], self.arr[1], self.arr[2]
        N = len(st)
        # the plan as the solver makes it for the graph WITH the knob: one more unary factor (which adds no edge, wherever it sits) and the
        # poses' x, y as the ordering's geometric hint (prepare_plan); tests/test_gpu_not_spd.py checks param->ordering against `perm`
        self.P = P = PlanView(lib, N, np.append(fa, 0), np.append(fb, -1), xy=np.asarray(st, float)[:, :2], leaf_nodes=leaf_nodes)
        A, b = dense_normal(self.arr, lam)
        pos = P.pos.astype(int)
        idx = np.empty(3 * N, int)                      # idx[p] = node-order scalar index of elimination position p
        for k in range(N):
            idx[3 * pos[k]:3 * pos[k] + 3] = 3 * k + np.arange(3)
        self.idx = idx
        self.node_of = np.empty(N, int); self.node_of[pos] = np.arange(N)
        self.A0 = A[np.ix_(idx, idx)]; self.b = b[idx]
        L = np.linalg.cholesky(self.A0)
        self.d = np.diag(L) ** 2
        self.first = 3 * P.front_first.astype(int); self.ns = 3 * P.front_nsb.astype(int); self.level = P.front_level.astype(int)
        self.n = 3 * N

    def s_star(self, p):
        e = np.zeros(self.n); e[p] = 1.0
        return 1.0 / float(np.linalg.solve(self.A0, e)[p])

    def classes(self):
        """class -> (front t, column c) for every class this graph offers under this plan (the first front that offers it)"""
        out = {}
        nF = len(self.first)
        top = int(self.level.max())
        last_front = int(np.argmax(self.first))
        for t in range(nF):
            ns, lev = int(self.ns[t]), int(self.level[t])
            offers = {}
            if lev == 0:
                offers["leaf_c0"] = 0
            if ns > 16:
                offers["blk_first"] = 16
            if ns >= 16:
                offers["blk_last"] = 15
            if ns >= 4:
                offers["interior"] = min(ns - 2, 5)
            if ns % 16 != 0 and t != last_front:
                offers["partial_last"] = ns - 1
            if 0 < lev < top and ns >= 4:
                offers["middle_level"] = min(ns - 2, 4)
            if t == last_front:
                offers["root_last"] = ns - 1
            if ns > 128:
                offers["big_ob0_p0_m0"] = 0
                offers["big_ob0_p3_m31"] = 127
                if ns > 128 + 7:
                    offers["big_ob1_p0_mid"] = 128 + 7
                if ns > 128 + 96:
                    offers["big_ob1_p3_m0"] = 128 + 96
                if ns % 32 != 0:
                    offers["big_partial_last"] = ns - 1
            for k, c in offers.items():
                out.setdefault(k, (t, c))
        return out

    def case(self, t, c, s_of=None, delta=DELTA):
        """the graph with the knob at column c of front t.  s_of(p, d_p) gives the knob's size (default (1 + delta) d_p).
        -> dict(arr, p, node, comp, s, d_p)"""
        p = int(self.first[t]) + c
        k, d = int(self.node_of[p // 3]), p % 3
        s = float(s_of(p, self.d[p])) if s_of else (1.0 + delta) * float(self.d[p])
        return dict(arr=with_knob(self.arr, k, d, s), p=p, node=k, comp=d, s=s, d_p=float(self.d[p]), front=t, col=c, graph=self.name,
                    diag=float(self.A0[p, p]) - s)

    def matrix(self, p, s):
        A = self.A0.copy(); A[p, p] -= s
        return A


@functools.lru_cache(maxsize=None)
def _placement(lib, name, leaf_nodes, lam):
    return Placement(lib, name, leaf_nodes, lam)


def placement(lib, name, leaf_nodes=16, lam=1e-4):
    return _placement(lib, name, int(leaf_nodes), float(lam))


def class_table(lib, leaf_nodes=16, lam=1e-4):
    """class -> (Placement, front, column): the first graph of GRAPHS that offers the class under this plan; and the missing classes"""
    tab = {}
    for name in GRAPHS:
        pl = placement(lib, name, leaf_nodes, lam)
        for k, (t, c) in pl.classes().items():
            tab.setdefault(k, (pl, t, c))
    return tab, [k for k in CLASSES if k not in tab]


def refined_solve(A, b, iters=40):
    """float64 LAPACK solve of the positive definite system A x = b (dpotrf / dpotrs, the routine for such a system and the factorisation
    the device computes) refined with residuals in longdouble until it stops changing -> (x_ref [longdouble], x_plain [float64]).
    Next to the edge of positive definiteness the plain solve's own deviation is one draw of a widely spread quantity: on the chain with the
    knob at (1 - 1e-8) s*, dpotrf and dgetrf in elimination and in node order deviate by 3.3e3 ... 1.4e6 from the refined solution
    (max |x| = 4.3e8) -- the same operations in another order."""
    import scipy.linalg as sla
    ch = sla.cho_factor(A, lower=True)
    x0 = sla.cho_solve(ch, b)
    Al = A.astype(np.longdouble); bl = b.astype(np.longdouble)
    x = x0.astype(np.longdouble)
    for _ in range(iters):
        r = bl - Al @ x
        xn = x + sla.cho_solve(ch, np.asarray(r, np.float64)).astype(np.longdouble)
        if np.array_equal(xn, x):
            break
        x = xn
    return x, x0
