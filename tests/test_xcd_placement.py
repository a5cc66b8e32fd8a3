"""Host logic (no GPU): the XCD placement of the batch step's multi-level launches (option xcd_place, plan.h: xcd_place).
Workgroup b runs on XCD class b % 8; a list is the level-ordered list permuted, with -1 in empty slots.  Checked here, on M3500's plan,
a random tree and the plan of a chain-like graph (deep and skewed): every list holds each front exactly once, every dependency has a
lower workgroup id (the invariant the flag waits need to be deadlock-free), no class holds more fronts than its cap, a front has the same
class in both sweeps, and the root's class holds a whole leaf-to-root path."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets
from tests.support.mf_emulator import PlanView

NX = 8


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _place(lib, parent, level, nsb, l0, cap, cap_leaf):
    f = lib.dll.aprilsam_amd_xcd_place
    parent, level, nsb = (np.ascontiguousarray(a, np.int32) for a in (parent, level, nsb))
    args = (len(parent), _ip(parent), _ip(level), _ip(nsb), l0, cap, cap_leaf)
    out = []
    for which in (0, 1, 2):
        n = f(*args, which, None, 0)
        assert n >= 0
        buf = np.zeros(max(n, 1), np.int32)
        assert f(*args, which, _ip(buf), n) == n
        out.append(buf[:n])
    return out + [f(*args, 3, None, 0)]


def _levels(parent):
    level = np.zeros(len(parent), np.int64)
    for t in range(len(parent)):                  # parents have higher ids
        if parent[t] >= 0:
            level[parent[t]] = max(level[parent[t]], level[t] + 1)
    return level


def _check(lib, parent, level, nsb, l0, cap, cap_leaf):
    parent, level = np.asarray(parent), np.asarray(level)
    up_l, dn_l, leaf_l, rc = _place(lib, parent, level, nsb, l0, cap, cap_leaf)
    assert rc == 0
    ml = sorted(np.nonzero(level >= l0)[0].tolist())
    leaves = sorted(np.nonzero(level == 0)[0].tolist()) if l0 == 1 else []
    for lst, members in ((up_l, ml), (dn_l, ml), (leaf_l, leaves)):
        assert len(lst) % NX == 0
        assert np.all(lst >= -1)
        assert sorted(lst[lst >= 0].tolist()) == members          # a permutation of the old list plus empty slots
    iu = {int(t): b for b, t in enumerate(up_l) if t >= 0}
    idn = {int(t): b for b, t in enumerate(dn_l) if t >= 0}
    for t in ml:
        p = int(parent[t])
        if p >= 0 and p in iu:
            assert iu[t] < iu[p]                                   # up: children first
            assert idn[p] < idn[t]                                 # down: parents first
        assert iu[t] % NX == idn[t] % NX                           # one class per front
    for lst, n, c in ((up_l, len(ml), cap), (leaf_l, len(leaves), cap_leaf)):
        if n <= NX * c:
            cnt = np.bincount(np.nonzero(lst >= 0)[0] % NX, minlength=NX)
            assert cnt.max() <= c
    # the critical path stays in one class: from the root, some child of the root's class at every step down to a front without children
    if ml and len(ml) <= NX * cap:
        root = max(ml, key=lambda t: level[t])
        kids = {}
        for t in ml:
            if parent[t] >= 0:
                kids.setdefault(int(parent[t]), []).append(t)
        t, c = root, iu[root] % NX
        while t in kids:
            same = [k for k in kids[t] if iu[k] % NX == c]
            assert same, f"front {t}: no child in the root's class"
            t = max(same, key=lambda k: level[k])
    return up_l, dn_l, leaf_l


def test_m3500_plan(lib):
    arr = datasets.m3500_batch()
    P = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], leaf_nodes=16)
    up_l, dn_l, leaf_l = _check(lib, P.front_parent, P.front_level, P.front_nsb, 1, 32, 64)
    n_ml = int((P.front_level >= 1).sum())
    # balanced classes: few empty slots, no class above an XCD's 32 compute units
    assert len(up_l) <= n_ml + 4 * NX and len(dn_l) <= n_ml + 4 * NX
    assert len(up_l) // NX <= 32
    # leaves run in their parent's class (the parent's extend-add reads them from its own L2)
    iu = {int(t): b % NX for b, t in enumerate(up_l) if t >= 0}
    same = sum(1 for b, t in enumerate(leaf_l) if t >= 0 and iu.get(int(P.front_parent[t]), -1) == b % NX)
    assert same >= 0.9 * int((leaf_l >= 0).sum())
    for l0 in (0, 2):
        _check(lib, P.front_parent, P.front_level, P.front_nsb, l0, 32, 64)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tree(lib, seed):
    rng = np.random.default_rng(seed)
    nF = int(rng.integers(50, 700))
    parent = np.full(nF, -1)
    for t in range(nF - 1):
        parent[t] = t + 1 + int(rng.integers(0, min(25, nF - 1 - t)))
    nsb = rng.integers(1, 40, nF)
    level = _levels(parent)
    for l0 in (0, 1, 2):
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


def test_star_and_chain_trees(lib):
    # star: one root, every other front a leaf; path: every front the only child of the next
    for parent in (np.r_[np.full(99, 99), -1], np.r_[np.arange(1, 120), -1]):
        level = _levels(parent)
        for l0 in (0, 1):
            _check(lib, parent, level, np.full(len(parent), 5), l0, 8, 8)


def test_selftest_covers_placement(lib):
    assert lib.dll.aprilsam_amd_selftest() == 0
