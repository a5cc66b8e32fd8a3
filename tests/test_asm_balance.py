"""Host logic (no GPU): which wave of a front's workgroup owns which block column in the extend-add (option asm_balance, plan.h: asm_owners).
The kernel gives every destination block column of a parent to one wave, which adds every child's contribution to it, child after child;
the time behind the wait for the children is set by the wave with the longest work list.  Column mod waves leaves the lists uneven; the plan
takes the columns by decreasing item count and gives each to the least loaded wave.  Checked here through the C entry point on M3500's plan and
on random trees: one owner per column, the same answer every time, no front's longest list longer than under the modulo rule, and on M3500 the
list lengths and trip counts the change was made for.

An item is what the kernel's fill loop queues: one per child block, one more where the block has a second 64-row pass (3 cnu + 1 - 3 jb > 64);
a trip takes TE = 4 items of one wave's list."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets
from tests.support.mf_emulator import PlanView

TE = 4


def _owners(lib, parent, nsb, nub, rows_ptr, rel, nw):
    f = lib.dll.aprilsam_amd_asm_owners
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    parent, nsb, nub, rel = (np.ascontiguousarray(a, np.int32) for a in (parent, nsb, nub, rel))
    rows_ptr = np.ascontiguousarray(rows_ptr, np.int64)
    own = np.full(max(len(rel), 1), -7, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    rc = f(len(parent), ip(parent), ip(nsb), ip(nub), rows_ptr.ctypes.data_as(C.POINTER(C.c_longlong)), ip(rel), nw, ip(own))
    assert rc == 0
    return own[:len(rel)]


def _lists(parent, nsb, nub, rows_ptr, rel, nw, own):
    """per parent front: (items per wave under the plan's owners, items per wave under column mod nw); checks one owner per column on the way"""
    nF = len(parent)
    col_owner = [dict() for _ in range(nF)]
    bal = np.zeros((nF, nw), np.int64); mod = np.zeros((nF, nw), np.int64)
    for t in range(nF):
        p = int(parent[t])
        for jb in range(int(nub[t])):
            e = int(rows_ptr[t]) + jb
            if p < 0:
                assert own[e] == -1
                continue
            b = int(rel[e]); w = int(own[e])
            assert 0 <= w < nw, (t, jb, w)                                   # an owner in [0, NW)
            assert col_owner[p].setdefault(b, w) == w, (p, b)              # ... and the same one for every child block of the column
            items = 1 + (3 * int(nub[t]) + 1 - 3 * jb > 64)
            bal[p, w] += items; mod[p, b % nw] += items
    return bal, mod


def _trips(lists):
    return int(((lists.max(axis=1) + TE - 1) // TE).sum())


def _check(lib, parent, nsb, nub, rows_ptr, rel, nw):
    own = _owners(lib, parent, nsb, nub, rows_ptr, rel, nw)
    assert np.array_equal(own, _owners(lib, parent, nsb, nub, rows_ptr, rel, nw))      # deterministic
    bal, mod = _lists(parent, nsb, nub, rows_ptr, rel, nw, own)
    assert np.array_equal(bal.sum(axis=1), mod.sum(axis=1))
    worse = np.nonzero(bal.max(axis=1) > mod.max(axis=1))[0]
    assert len(worse) == 0, (nw, worse[:5], bal[worse[:5]].max(axis=1), mod[worse[:5]].max(axis=1))      # never longer than under the modulo rule
    return bal, mod


@pytest.fixture(scope="module")
def m3500(lib):
    arr = datasets.m3500_batch()
    return PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], leaf_nodes=16)


def test_m3500_lists_of_the_critical_path_at_16_waves(lib, m3500):
    P = m3500
    bal, mod = _check(lib, P.front_parent, P.front_nsb, P.front_nub, P.front_rows_ptr, P.front_rel, 16)
    got = {t: (int(mod[t].max()), int(bal[t].max())) for t in (45, 46, 50, 98, 166, 354, 679)}
    print(f"[asm_balance] M3500, 16 waves, longest list (mod 16, balanced): {got}")
    for t, most in zip((45, 46, 50, 98, 166, 354, 679), (3, 5, 6, 5, 6, 4, 2)):
        assert bal[t].max() <= most, (t, bal[t].max(), most)


@pytest.mark.parametrize("nw,most", [(16, 209), (8, 245), (4, 409)])
def test_m3500_trips_over_all_fronts(lib, m3500, nw, most):
    P = m3500
    bal, mod = _check(lib, P.front_parent, P.front_nsb, P.front_nub, P.front_rows_ptr, P.front_rel, nw)
    print(f"[asm_balance] M3500, {nw} waves: trips {_trips(mod)} under column mod waves, {_trips(bal)} balanced")
    assert _trips(bal) <= most


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tree(lib, seed):
    """the trees of test_up_schedule.py, with block maps drawn at random: every child's update blocks map, strictly increasing, into its parent's
    columns (so a child has at most as many update blocks as its parent has columns)"""
    rng = np.random.default_rng(seed)
    nF = int(rng.integers(50, 700))
    parent = np.full(nF, -1)
    for t in range(nF - 1):
        parent[t] = t + 1 + int(rng.integers(0, min(25, nF - 1 - t)))
    nsb = rng.integers(1, 40, nF)
    nub = np.zeros(nF, np.int64)
    maps = [None] * nF
    for t in range(nF - 1, -1, -1):                                   # parents have higher ids: parents first
        p = int(parent[t])
        if p < 0:
            maps[t] = np.zeros(0, np.int64); continue
        nbc = int(nsb[p] + nub[p])
        nub[t] = int(rng.integers(1, min(nbc, 60) + 1))              # (tall children too: more than 21 blocks gives second passes)
        maps[t] = np.sort(rng.choice(nbc, int(nub[t]), replace=False))
    rows_ptr = np.r_[0, np.cumsum(nub)]
    rel = np.concatenate(maps)
    for nw in (4, 8, 16):
        _check(lib, parent, nsb, nub, rows_ptr, rel, nw)


def test_arguments_that_are_no_tree_are_refused(lib):
    f = lib.dll.aprilsam_amd_asm_owners
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    parent, nsb, nub, rel = np.array([0, -1], np.int32), np.array([2, 3], np.int32), np.array([1, 0], np.int32), np.array([0], np.int32)      # front 0 its own parent
    rows_ptr = np.array([0, 1, 1], np.int64); own = np.zeros(1, np.int32)
    assert f(2, ip(parent), ip(nsb), ip(nub), rows_ptr.ctypes.data_as(C.POINTER(C.c_longlong)), ip(rel), 4, ip(own)) == -100
    parent[0] = 1
    assert f(2, ip(parent), ip(nsb), ip(nub), rows_ptr.ctypes.data_as(C.POINTER(C.c_longlong)), ip(rel), 0, ip(own)) == -100       # no waves
    assert f(2, ip(parent), ip(nsb), ip(nub), rows_ptr.ctypes.data_as(C.POINTER(C.c_longlong)), ip(rel), 4, ip(own)) == 0 and own[0] == 0
    rows_ptr -= 1                                                                                                                  # entries before rel and owner
    own[0] = 7
    assert f(2, ip(parent), ip(nsb), ip(nub), rows_ptr.ctypes.data_as(C.POINTER(C.c_longlong)), ip(rel), 4, ip(own)) == -100 and own[0] == 7
