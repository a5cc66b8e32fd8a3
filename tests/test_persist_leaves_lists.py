"""Host logic (no GPU): the list of the back substitution's multi-level launch when level 0 joins it (option persist_leaves, plan.h:
dn_with_leaves).  The leaves' workgroups follow the upper fronts': checked here, on M3500's plan, random trees, a star, a path and the plan
of a chain-like graph, for the level-ordered list and for the XCD-placed one: the list holds every front of
the tree exactly once plus -1 padding, every parent has a lower workgroup id than its children (what keeps the waits deadlock-free), the
upper fronts sit in the very slots of today's down-sweep list, and a front keeps one XCD class (id % 8) in both sweeps -- an upper front
the class of the up-sweep's list, a leaf the class of level 0's own list, which the factorisation still launches."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets
from tests.support.mf_emulator import PlanView

NX = 8


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _call(f, args, which):
    n = f(*args, which, None, 0)
    assert n >= 0
    buf = np.zeros(max(n, 1), np.int32)
    assert f(*args, which, _ip(buf), n) == n
    return buf[:n]


def _levels(parent):
    level = np.zeros(len(parent), np.int64)
    for t in range(len(parent)):                  # parents have higher ids
        if parent[t] >= 0:
            level[parent[t]] = max(level[parent[t]], level[t] + 1)
    return level


def _check(lib, parent, level, nsb, cap, cap_leaf):
    parent, level, nsb = (np.ascontiguousarray(a, np.int32) for a in (parent, level, nsb))
    nF = len(parent)
    join = (nF, _ip(parent), _ip(level), _ip(nsb), cap, cap_leaf)
    place = (nF, _ip(parent), _ip(level), _ip(nsb), 1, cap, cap_leaf)
    up_l, dn_l, leaf_l = (_call(lib.dll.aprilsam_amd_xcd_place, place, w) for w in (0, 1, 2))
    upper = [t for l in range(1, int(level.max()) + 1) for t in np.nonzero(level == l)[0].tolist()][::-1]      # the level-ordered list backwards: parents first
    leaves = np.nonzero(level == 0)[0].tolist()
    out = {}
    for which in (0, 1):
        lst = _call(lib.dll.aprilsam_amd_persist_leaves_list, join, which)
        assert lib.dll.aprilsam_amd_persist_leaves_list(*join, which + 2, None, 0) == 0
        assert np.all(lst >= -1)
        assert sorted(lst[lst >= 0].tolist()) == list(range(nF))          # every front of the tree once, the rest padding
        idn = {int(t): b for b, t in enumerate(lst) if t >= 0}
        for t in range(nF):
            if parent[t] >= 0:
                assert idn[int(parent[t])] < idn[t], (which, t)           # parents first
        if which == 0:
            assert lst.tolist() == upper + leaves                         # today's parents-first list, then level 0's
        else:
            assert len(lst) == len(dn_l) + len(leaf_l) and len(dn_l) % NX == 0 and len(leaf_l) % NX == 0
            assert np.array_equal(lst[:len(dn_l)], dn_l)                  # the upper fronts' slots do not move
            cls_up = {int(t): b % NX for b, t in enumerate(up_l) if t >= 0}
            cls_up.update({int(t): b % NX for b, t in enumerate(leaf_l) if t >= 0})
            for t in range(nF):
                assert idn[t] % NX == cls_up[t], (which, t)               # one class per front in both sweeps
            assert np.array_equal(lst[len(dn_l):], leaf_l)                # ... and the leaves follow in the slots of their own list
        out[which] = lst
    return out


def test_m3500_plan(lib):
    arr = datasets.m3500_batch()
    P = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], leaf_nodes=16)
    out = _check(lib, P.front_parent, P.front_level, P.front_nsb, 32, 64)
    n_up, n_leaf = int((P.front_level >= 1).sum()), int((P.front_level == 0).sum())
    assert len(out[0]) == n_up + n_leaf
    assert len(out[1]) <= n_up + n_leaf + 8 * NX                          # few empty slots: the launch stays about as large as its fronts


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tree(lib, seed):
    rng = np.random.default_rng(seed)
    nF = int(rng.integers(50, 700))
    parent = np.full(nF, -1)
    for t in range(nF - 1):
        parent[t] = t + 1 + int(rng.integers(0, min(25, nF - 1 - t)))
    nsb = rng.integers(1, 40, nF)
    for cap in (4, 32):
        _check(lib, parent, _levels(parent), nsb, cap, cap)


def test_star_and_path(lib):
    # star: one root, every other front a leaf; path: every front the only child of the next (one leaf)
    for parent in (np.r_[np.full(99, 99), -1], np.r_[np.arange(1, 120), -1]):
        _check(lib, parent, _levels(parent), np.full(len(parent), 5), 8, 8)


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
    for cap in (2, 32):
        _check(lib, P.front_parent, P.front_level, P.front_nsb, cap, cap)


def test_selftest_covers_the_lists(lib):
    assert lib.dll.aprilsam_amd_selftest() == 0
