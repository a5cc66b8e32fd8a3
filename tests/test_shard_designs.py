"""The designed sharded runs, without a GPU: every (graph, world) of tests/support/shard_designs.py reaches exactly the classes it declares
on the library's own plan and ownership map (aprilsam_amd_shard_plan), every class is reached, the pool arithmetic of the design module
agrees with the plan's -- and tests/support/thread_comm.py alone: W threads move numpy buffers along a plan's exchange schedule, the
ordered all-reduce is bitwise equal on every rank, and a missing sender or a missing rank gives return code 1 within the timeout."""
import time

import numpy as np
import pytest

from tests.support import shard_designs as D
from tests.support import thread_comm as TC


@pytest.mark.parametrize("entry", D.ALL, ids=D.ident)
def test_entry_reaches_exactly_what_it_declares(lib, entry):
    name, world = entry
    got = D.classes_of(lib, name, world)
    assert got == D.declared(name, world), (entry, got)
    assert all(c in D.CLASSES for c in got)


def test_every_class_is_reached_and_every_graph_has_its_worlds():
    reached = {c for name, w in D.ALL for c in D.declared(name, w)}
    assert reached == set(D.CLASSES), set(D.CLASSES) - reached
    assert set(D.ENTRIES) == set(D.GRAPHS)
    for name in D.GRAPHS:
        assert tuple(D.ENTRIES[name]) == D.worlds_of(name), name
    # odd worlds and idle ranks on the data path, not only on single-front graphs: an entry with transfers AND the class
    assert any({"odd", "prim"} <= set(D.declared(n, w)) for n, w in D.ALL) and any({"idle", "prim"} <= set(D.declared(n, w)) for n, w in D.ALL)


def test_option_entries_hold_what_they_are_there_for():
    ent = D.OPTION_ENTRIES
    assert len(ent) > 80 and all("prim" in D.declared(*e) for e in ent)
    assert any("u>TPB" in D.declared(*e) for e in ent) and any("half" in D.declared(*e) for e in ent) and any("refill" in D.declared(*e) for e in ent)
    assert all(e in D.ALL for e in D.THREE_ITERATIONS)


@pytest.mark.parametrize("name", ["6,5 x2", "mixed leaves 200,130,64 under 64", "two_components"])
def test_pool_arithmetic_world_one_is_the_whole_plan(lib, name):
    """Map.pool_doubles restates shard_begin's layout; with one rank it must give the plan's own pool (front_off of the last front + its array)"""
    P = D.plan(lib, name)
    M = D.Map(P, 1)
    last = int(np.argmax(P.front_off))
    m = 3 * int(P.front_nsb[last] + P.front_nub[last])
    assert not M.ghost.any() and M.pool_doubles(0) == int(P.front_off[last]) + (m + 3) * m
    for w in D.worlds_of(name):
        Mw = D.Map(P, w)
        own = sum(Mw.pool_doubles(r) for r in range(w))
        ghosts = sum((3 * int(P.front_nub[t]) + 3) * 3 * int(P.front_nub[t]) for t in np.flatnonzero(Mw.ghost))
        assert M.pool_doubles(0) - 32 * P.nF <= own - ghosts <= M.pool_doubles(0) + 32 * (P.nF + len(Mw.xfer)), (name, w)
        assert all(Mw.pool_doubles(r) == 0 for r in range(w) if r not in set(Mw.owner.tolist()))


# ------------------------------------------------------------------------------------------------------
# thread_comm alone
# ------------------------------------------------------------------------------------------------------
def _walk(fabric, rank, P, world, n):
    """the schedule of expected_log through the fabric's own callbacks, payload = the front id; returns what arrived"""
    cb = fabric.host_comm(rank)
    xfer, bcast, owner = P.shard[world]
    got = []

    def dp(a):
        import ctypes as C
        return a.ctypes.data_as(C.POINTER(C.c_double))
    one = np.array([float(rank + 1)])
    assert cb.allreduce_sum(None, dp(one), 1) == 0
    got.append(("sum", one[0]))
    for l in range(P.nLevels):
        for lev, front, src, dst, _, cnt in xfer[xfer[:, 0] == l]:
            buf = np.full(int(cnt), float(front) if rank == src else -1.0)
            if rank == src:
                assert cb.send(None, dp(buf), int(cnt), int(dst)) == 0
            elif rank == dst:
                assert cb.recv(None, dp(buf), int(cnt), int(src)) == 0
                assert np.all(buf == float(front))
                got.append(("recv", int(front)))
    for l in range(P.nLevels - 1, -1, -1):
        for lev, front, own, first, nsb in bcast[bcast[:, 0] == l]:
            buf = np.full(3 * int(nsb), float(front) if rank == own else -1.0)
            assert cb.bcast(None, dp(buf), 3 * int(nsb), int(own)) == 0
            assert np.all(buf == float(front))
    for k in (1, 1, 9 * n):
        buf = np.full(k, float(rank))
        assert cb.allreduce_sum(None, dp(buf), k) == 0
        assert np.all(buf == float(sum(range(world))))
    return got


@pytest.mark.parametrize("entry", [("6,5 x65", 3), ("two_components", 5), ("30,25,20 fan 2", 8)], ids=D.ident)
def test_threads_walk_a_plans_schedule(lib, entry):
    name, world = entry
    P = D.plan(lib, name)
    fabric = TC.Fabric(world)
    res = TC.run_threads(world, lambda r: _walk(fabric, r, P, world, P.N))
    xfer, bcast, owner = P.shard[world]
    for r in range(world):
        assert res[r][0] == ("sum", float(sum(range(1, world + 1))))
        assert sorted(f for k, f in res[r][1:]) == sorted(int(x[1]) for x in xfer if x[3] == r)
        assert fabric.log[r] == TC.expected_log(r, world, xfer, bcast, P.nLevels, P.N) and set(fabric.rcs[r]) == {0}
        assert sum(1 for k in fabric.log[r] if k[0] == "bcast") == len(bcast)          # every rank takes part in every broadcast, the idle ones too
    assert all(q.empty() for q in fabric.q.values())


@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_ordered_allreduce_is_bitwise_equal_on_every_rank(world):
    rng = np.random.default_rng(world)
    data = [rng.normal(size=1000) * 10.0 ** rng.integers(-12, 12, 1000) for _ in range(world)]
    fabric = TC.Fabric(world)

    def body(r):
        buf = data[r].copy()
        fabric.allreduce_sum(r, buf)
        return buf
    res = TC.run_threads(world, body)
    want = data[0].copy()
    for r in range(1, world):
        want += data[r]
    if world > 2:                                  # (the order matters for this data: the other order gives other bits)
        back = data[-1].copy()
        for r in range(world - 2, -1, -1):
            back += data[r]
        assert not np.array_equal(want, back)
    for r in range(world):
        assert np.array_equal(res[r], want)
    # ... and x + 0 + ... + 0 is exact wherever x sits
    for k in range(world):
        f2 = TC.Fabric(world)
        res = TC.run_threads(world, lambda r: (lambda b: (f2.allreduce_sum(r, b), b)[1])(data[0].copy() if r == k else np.zeros(1000)))
        assert all(np.array_equal(v, data[0]) for v in res)


def test_a_missing_sender_and_a_missing_rank_give_1_within_the_timeout():
    import ctypes as C
    fabric = TC.Fabric(2, timeout=0.2)
    cb = fabric.host_comm(1)
    buf = np.zeros(4)
    t0 = time.monotonic()
    assert cb.recv(None, buf.ctypes.data_as(C.POINTER(C.c_double)), 4, 0) == 1          # nobody sends
    assert cb.allreduce_sum(None, buf.ctypes.data_as(C.POINTER(C.c_double)), 4) == 1    # rank 0 never arrives
    assert cb.bcast(None, buf.ctypes.data_as(C.POINTER(C.c_double)), 4, 0) == 1         # (a broken barrier answers at once)
    assert time.monotonic() - t0 < 5.0
    assert fabric.log[1] == [("recv", 4, 0), ("allreduce", 4, -1), ("bcast", 4, 0)] and fabric.rcs[1] == [1, 1, 1]
    # a wrong count is an error, not a short copy; an injected failure moves nothing
    f2 = TC.Fabric(2, timeout=0.2)
    a, b = f2.host_comm(0), f2.host_comm(1)
    src = np.arange(3.0); dst = np.zeros(4)
    assert a.send(None, src.ctypes.data_as(C.POINTER(C.c_double)), 3, 1) == 0
    assert b.recv(None, dst.ctypes.data_as(C.POINTER(C.c_double)), 4, 0) == 1 and not dst.any()
    f2.inject.add((0, "send"))
    assert a.send(None, src.ctypes.data_as(C.POINTER(C.c_double)), 3, 1) == 1 and f2.q[(0, 1)].empty()
    assert a.send(None, src.ctypes.data_as(C.POINTER(C.c_double)), 3, 1) == 0              # (the next one goes through)


def test_an_exception_of_a_rank_reaches_the_main_thread():
    def body(r):
        if r == 1:
            raise KeyError("rank 1")
        return r
    with pytest.raises(KeyError):
        TC.run_threads(3, body)
