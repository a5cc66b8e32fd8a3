"""Host logic (no GPU): the order of the factorisation's one launch once level 0 is inside it (option persist_up, plan.h: up_schedule).
Dispatch follows the workgroup ids, so the list IS the schedule: mode 2 orders the fronts by their remaining path to the root under the cost
model, mode 3 by a list schedule that knows how many workgroups an XCD class holds at once.  Checked here through the C entry point, on
M3500's plan, random trees, the plan of a chain-like graph, a star and a path: the list holds every front of the level-ordered list once,
in the class it has there (and so in the back substitution's list), every child at a lower id than its parent (what keeps the flag waits
deadlock-free), the padding within the bound the slot rule guarantees, and under the model never behind level order.

The padding bound: the k-th front emitted takes a slot of round k at the latest (its class's last round and its children's rounds all
belong to fronts emitted before it), so a list of n fronts has at most 8 n slots -- reached by a path, whose fronts share one class."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets
from tests.support.mf_emulator import PlanView

NX = 8
HAND, PERCOL, LEAF = 12.0, 0.19, 4.8            # the committed cost model (plan.h; profiles/persist_leaves.txt section 5), us
MODES = (2, 3)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _list(f, args, which):
    n = f(*args, which, None, 0)
    assert n >= 0
    buf = np.zeros(max(n, 1), np.int32)
    assert f(*args, which, _ip(buf), n) == n
    return buf[:n]


def _base(lib, parent, level, nsb, l0, cap, cap_leaf):
    """the level-ordered list of the one launch: the placed leaf list, then the upper fronts' (l0 = 1), or the whole tree's placed list (l0 = 0)"""
    args = (len(parent), _ip(parent), _ip(level), _ip(nsb), l0, cap, cap_leaf)
    up_l = _list(lib.dll.aprilsam_amd_xcd_place, args, 0)
    leaf_l = _list(lib.dll.aprilsam_amd_xcd_place, args, 2)
    return np.ascontiguousarray(np.r_[leaf_l, up_l], np.int32)


def _schedule(lib, parent, nsb, base, cap, mode):
    """(list, checker's code, the model's makespan of the list)"""
    f = lib.dll.aprilsam_amd_up_schedule
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double)]
    span = C.c_double(-2.0)
    args = (len(parent), _ip(parent), _ip(nsb), _ip(base), len(base), cap, mode)
    n = f(*args, 0, None, 0, None)
    assert n >= 0
    buf = np.zeros(max(n, 1), np.int32)
    assert f(*args, 0, _ip(buf), n, C.byref(span)) == n
    return buf[:n], f(*args, 1, None, 0, None), span.value


def _priorities(parent, nsb, members):
    inside = np.zeros(len(parent), bool); inside[members] = True
    has_kids = np.zeros(len(parent), bool)
    for t in members:
        if parent[t] >= 0 and inside[parent[t]]:
            has_kids[parent[t]] = True
    cost = np.where(has_kids, HAND + PERCOL * 3.0 * nsb, LEAF)
    prio = np.zeros(len(parent))
    for t in sorted(members, reverse=True):                        # parents have higher ids: parents first
        prio[t] = cost[t] + (prio[parent[t]] if parent[t] >= 0 and inside[parent[t]] else 0.0)
    return prio, has_kids


def _levels(parent):
    level = np.zeros(len(parent), np.int64)
    for t in range(len(parent)):
        if parent[t] >= 0:
            level[parent[t]] = max(level[parent[t]], level[t] + 1)
    return level


def _check(lib, parent, level, nsb, l0, cap, cap_leaf):
    parent, level, nsb = (np.ascontiguousarray(a, np.int32) for a in (parent, level, nsb))
    base = _base(lib, parent, level, nsb, l0, cap, cap_leaf)
    members = sorted(base[base >= 0].tolist())
    assert members == list(range(len(parent)))                     # the whole tree is in the launch
    want = {int(t): b % NX for b, t in enumerate(base) if t >= 0}
    if l0 == 1:                                                    # ... which is the class of the back substitution's list with the leaves inside
        dn = _list(lib.dll.aprilsam_amd_persist_leaves_list, (len(parent), _ip(parent), _ip(level), _ip(nsb), cap, cap_leaf), 1)
        assert want == {int(t): b % NX for b, t in enumerate(dn) if t >= 0}
    _, rc0, span0 = _schedule(lib, parent, nsb, base, cap, 0)
    assert rc0 == 0 and span0 > 0
    out = {}
    for mode in MODES:
        lst, rc, span = _schedule(lib, parent, nsb, base, cap, mode)
        assert rc == 0, (mode, rc)
        assert len(lst) % NX == 0 and np.all(lst >= -1)
        assert sorted(lst[lst >= 0].tolist()) == members          # a permutation of all fronts plus empty slots
        ids = {int(t): b for b, t in enumerate(lst) if t >= 0}
        for t in members:
            if parent[t] >= 0:
                assert ids[t] < ids[int(parent[t])], (mode, t)     # every child below its parent
            assert ids[t] % NX == want[t], (mode, t)               # the class it was given
        assert len(lst) <= NX * len(members)                       # the padding bound (module docstring)
        print(f"[up_schedule] fronts {len(members)} l0 {l0} cap {cap} mode {mode}: {len(lst)} slots, makespan {span:.1f} us against level order {span0:.1f} us")
        assert 0 < span <= span0, (mode, span, span0)              # under the model never behind level order
        out[mode] = (lst, ids, span)
    return base, out


def test_m3500_plan(lib):
    arr = datasets.m3500_batch()
    P = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], leaf_nodes=16)
    parent, level, nsb = np.asarray(P.front_parent), np.asarray(P.front_level), np.asarray(P.front_nsb)
    cap = 32                                                       # one workgroup per compute unit, 32 units per XCD
    base, out = _check(lib, parent, level, nsb, 1, cap, 64)
    _check(lib, parent, level, nsb, 0, cap, cap)
    prio, _ = _priorities(parent, nsb, list(range(len(parent))))
    leaves = np.nonzero(level == 0)[0]
    crit = int(leaves[np.argmax(prio[leaves])])
    path = [crit]
    while parent[path[-1]] >= 0:
        path.append(int(parent[path[-1]]))
    kids = {}
    for t in range(len(parent)):
        if parent[t] >= 0:
            kids.setdefault(int(parent[t]), []).append(t)
    for mode in MODES:
        lst, ids, span = out[mode]
        print(f"[up_schedule] M3500 mode {mode}: critical leaf {crit} at id {ids[crit]}, path ids {[ids[t] for t in path]}")
        assert ids[crit] < NX * cap, (mode, ids[crit])             # the critical leaf is dispatched in the first round of slots
        for t in path[1:]:
            last = max(ids[k] for k in kids[t])
            assert last < ids[t] <= last + NX * cap, (mode, t, last, ids[t])      # no more than one round of slots behind its last child


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tree(lib, seed):
    rng = np.random.default_rng(seed)
    nF = int(rng.integers(50, 700))
    parent = np.full(nF, -1)
    for t in range(nF - 1):
        parent[t] = t + 1 + int(rng.integers(0, min(25, nF - 1 - t)))
    nsb = rng.integers(1, 40, nF)
    level = _levels(parent)
    for l0 in (0, 1):
        for cap in (4, 32):
            _check(lib, parent, level, nsb, l0, cap, cap)


def test_chain_like_graph(lib):
    """odometry chain with sparse loop closures: a deep, skewed assembly tree"""
    N = 1500
    fa = list(range(N - 1)); fb = list(range(1, N))
    rng = np.random.default_rng(7)
    for _ in range(40):
        a = int(rng.integers(0, N - 50)); fa.append(a); fb.append(a + int(rng.integers(10, 50)))
    fa, fb = np.array(fa), np.array(fb)
    xy = np.column_stack([np.cos(np.arange(N) * 0.01) * np.arange(N), np.sin(np.arange(N) * 0.01) * np.arange(N)])
    P = PlanView(lib, N, fa, fb, xy=xy, leaf_nodes=16)
    assert P.nLevels >= 3
    for l0 in (0, 1):
        for cap in (2, 32):
            _check(lib, P.front_parent, P.front_level, P.front_nsb, l0, cap, cap)


def test_star_and_path_trees(lib):
    # star: one root, every other front a leaf; path: every front the only child of the next
    for parent in (np.r_[np.full(99, 99), -1], np.r_[np.arange(1, 120), -1]):
        level = _levels(parent)
        for l0 in (0, 1):
            _check(lib, parent, level, np.full(len(parent), 5), l0, 8, 8)


def test_makespan_of_a_list_that_is_no_schedule(lib):
    """a parent at a lower id than its child: the checker names it and the model gives no makespan"""
    parent, nsb = np.array([2, 2, -1], np.int32), np.array([3, 3, 3], np.int32)
    base = np.array([0, 1, -1, -1, -1, -1, -1, -1, 2, -1, -1, -1, -1, -1, -1, -1], np.int32)
    bad = np.array([2, 1, -1, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1, -1], np.int32)
    _, rc, span = _schedule(lib, parent, nsb, base, 4, 0)
    assert rc == 0 and span == pytest.approx(LEAF + HAND + PERCOL * 9)         # both leaves at once, the root's prelude hidden behind them
    _, rc, span = _schedule(lib, parent, nsb, bad, 4, 0)
    assert rc == -4 and span == -1.0


def test_selftest_covers_the_schedule(lib):
    assert lib.dll.aprilsam_amd_selftest() == 0
