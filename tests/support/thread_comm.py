"""The ranks of a sharded solve as THREADS of one process.  TEST-ONLY.

aprilsam_amd_host_comm_t is four blocking callbacks, and the library may be driven from several threads on different device slots
(tests/test_gpu_slots.py: no process-globals), so W ranks are W threads, each with its own graph and its own param bound to slot `rank`
(aprilsam_amd_param_set_device before shard_begin).  One process holds the GPU and there is no process group to set up: a case takes
seconds where tests/test_gpu_shard.py (spawned processes over gloo: the only tests on the gloo and RCCL wires) takes tens of seconds.

The transport (`Fabric`): send / recv go through one queue per (src, dst); bcast and allreduce through a barrier and a shared slot.  The
all-reduce adds IN RANK ORDER on every rank: the library's gather relies on x + 0 + ... + 0 being exact and the tests compare the ranks'
results bit for bit.  Nothing waits for ever: every queue get and every barrier wait takes `Fabric.timeout` (TIMEOUT by default); on a
timeout the callback returns 1, the library leaves with -6 and the other ranks time out in turn.  Every callback is logged per rank as
(kind, count, peer or root; -1 for an all-reduce), so that a test can hold the schedule the LIBRARY executed to aprilsam_amd_shard_info
of the same run (`expected_log`).

The driver (`run`): one thread per rank runs `body(rank_handle)`; results come back per rank, exceptions are re-raised on the main
thread.  The joins are bounded; after a join that timed out, or after any rank reported a HIP error, the module refuses to start
another run (`assert_usable`): nothing more goes to a device that may have faulted.  Options are process-wide: set them on the main
thread around `run`, never from a body."""
import ctypes as C
import queue
import threading

import numpy as np

from aprilsam_amd.shard import _ALLRED, _BCAST, _RECV, _SEND, HostComm

TIMEOUT = 60.0                  # seconds: every queue get and every barrier wait
JOIN_TIMEOUT = 4 * TIMEOUT      # a rank thread: a few waits that time out one after the other, at the worst
ERR_HIP = -10                   # csrc/errors.h
_UNUSABLE = []                  # why no further run may start (a hung thread, a HIP error)


def assert_usable():
    assert not _UNUSABLE, f"an earlier sharded run left the device in doubt, nothing more is started on it: {_UNUSABLE[0]}"


class Fabric:
    """the wires between `world` rank threads"""

    def __init__(self, world, timeout=TIMEOUT):
        self.world, self.timeout = int(world), float(timeout)
        self.q = {(s, d): queue.Queue() for s in range(world) for d in range(world) if s != d}
        self.barrier = threading.Barrier(world)
        self.slot = [None] * world
        self.log = [[] for _ in range(world)]
        self.rcs = [[] for _ in range(world)]              # what every callback returned, in step with log
        self.inject = set()                                # (rank, kind): that rank's NEXT callback of that kind returns 1 and moves nothing

    def _wait(self):
        self.barrier.wait(self.timeout)                    # (raises BrokenBarrierError on a timeout, and from then on at once)

    def _guard(self, rank, kind, count, peer, fn):
        self.log[rank].append((kind, int(count), int(peer)))
        rc = 1
        try:
            if (rank, kind) in self.inject:
                self.inject.discard((rank, kind))
            else:
                fn()
                rc = 0
        except (queue.Empty, threading.BrokenBarrierError, ValueError):
            rc = 1
        except BaseException:                              # noqa: BLE001 -- never let an exception cross the C boundary
            rc = 2
        self.rcs[rank].append(rc)
        return rc

    # -- the four operations, on numpy views of the caller's buffer -------------------------------------------------------------------
    def send(self, rank, buf, dst):
        if not (0 <= dst < self.world) or dst == rank:
            raise ValueError("bad peer")
        self.q[(rank, dst)].put(buf.copy())

    def recv(self, rank, buf, src):
        if not (0 <= src < self.world) or src == rank:
            raise ValueError("bad peer")
        got = self.q[(src, rank)].get(timeout=self.timeout)
        if got.shape != buf.shape:
            raise ValueError("count mismatch")
        buf[:] = got

    def bcast(self, rank, buf, root):
        if not 0 <= root < self.world:
            raise ValueError("bad root")
        if rank == root:
            self.slot[root] = buf.copy()
        self._wait()
        if rank != root:
            if self.slot[root].shape != buf.shape:
                raise ValueError("count mismatch")
            buf[:] = self.slot[root]
        self._wait()                                       # (nobody overwrites the slot before everybody has read it)

    def allreduce_sum(self, rank, buf):
        self.slot[rank] = buf.copy()
        self._wait()
        if any(s.shape != buf.shape for s in self.slot):
            raise ValueError("count mismatch")
        acc = self.slot[0].copy()
        for r in range(1, self.world):                     # rank order, on every rank: bitwise the same sum everywhere
            acc += self.slot[r]
        self._wait()
        buf[:] = acc

    def host_comm(self, rank):
        """the aprilsam_amd_host_comm_t of one rank (keep the returned object alive as long as the library may call it)"""
        def view(p, n):
            return np.ctypeslib.as_array(p, shape=(int(n),))
        return HostComm(None,
                        _SEND(lambda u, p, n, dst: self._guard(rank, "send", n, dst, lambda: self.send(rank, view(p, n), int(dst)))),
                        _RECV(lambda u, p, n, src: self._guard(rank, "recv", n, src, lambda: self.recv(rank, view(p, n), int(src)))),
                        _BCAST(lambda u, p, n, root: self._guard(rank, "bcast", n, root, lambda: self.bcast(rank, view(p, n), int(root)))),
                        _ALLRED(lambda u, p, n: self._guard(rank, "allreduce", n, -1, lambda: self.allreduce_sum(rank, view(p, n)))))


def run_threads(world, body, join_timeout=JOIN_TIMEOUT):
    """body(rank) on `world` threads -> list of results; an exception of any rank is re-raised here"""
    out = [None] * world

    def main(rank):
        try:
            out[rank] = (True, body(rank))
        except BaseException as e:                         # noqa: BLE001 -- reported by the main thread
            out[rank] = (False, e)
    th = [threading.Thread(target=main, args=(r,), name=f"rank{r}", daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(join_timeout)
    hung = [t.name for t in th if t.is_alive()]
    if hung:
        _UNUSABLE.append(f"{hung} still running after {join_timeout} s")
        raise AssertionError(_UNUSABLE[-1])
    for r, (ok, v) in enumerate(out):
        if not ok:
            raise v
    return [v for _, v in out]


# ------------------------------------------------------------------------------------------------------
# the library's sharded calls, one handle per rank
# ------------------------------------------------------------------------------------------------------
def bind(lib):
    """argument types of the aprilsam_amd_shard_* entry points (as aprilsam_amd/shard.py declares them); main thread, once"""
    d = lib.dll
    d.aprilsam_amd_shard_info.restype = C.c_longlong
    d.aprilsam_amd_shard_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.c_longlong]
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    d.aprilsam_amd_shard_iterate.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    d.aprilsam_amd_shard_gather_states.argtypes = [C.c_void_p, C.c_void_p]
    d.aprilsam_amd_shard_chi2.restype = C.c_double
    d.aprilsam_amd_shard_chi2.argtypes = [C.c_void_p, C.c_void_p]
    d.aprilsam_amd_shard_comm_init_host.argtypes = [C.c_void_p, C.POINTER(HostComm)]
    d.aprilsam_amd_shard_end.argtypes = [C.c_void_p]


class Rank:
    """one rank of a run: its graph, its param on slot `rank`, its end of the fabric"""

    def __init__(self, lib, fabric, rank, arrays):
        self.lib, self.fabric, self.rank, self.world = lib, fabric, rank, fabric.world
        self.g = lib.new_graph(); self.g.build_from_arrays(*arrays); self.p = lib.new_param()
        assert lib.dll.aprilsam_amd_param_set_device(self.p.ptr, rank) == 0
        self._g = C.cast(self.g.ptr, C.c_void_p); self._p = C.cast(self.p.ptr, C.c_void_p)
        self._cb = None

    def _rc(self, rc):
        if rc == ERR_HIP:
            _UNUSABLE.append(f"rank {self.rank}: a HIP call failed: {self.lib.last_error()}")
        return int(rc)

    def begin(self):
        """shard_begin + the host-callback transport (world > 1) -> return code"""
        rc = self._rc(self.lib.dll.aprilsam_amd_shard_begin(self._g, self._p, self.rank, self.world))
        if rc == 0 and self.world > 1:
            self._cb = self.fabric.host_comm(self.rank)
            rc = self._rc(self.lib.dll.aprilsam_amd_shard_comm_init_host(self._p, C.byref(self._cb)))
        return rc

    def info(self, what):
        n = self.lib.dll.aprilsam_amd_shard_info(self._p, what, None, 0)
        out = np.zeros(max(int(n), 1), np.int64)
        self.lib.dll.aprilsam_amd_shard_info(self._p, what, out.ctypes.data_as(C.POINTER(C.c_longlong)), n)
        return out[:max(int(n), 0)]

    def iterate(self, n=1):
        return self._rc(self.lib.dll.aprilsam_amd_shard_iterate(self._g, self._p, int(n)))

    def chi2(self):
        v = float(self.lib.dll.aprilsam_amd_shard_chi2(self._g, self._p))
        if v != v and self.lib.last_error()[0] == ERR_HIP:         # (chi2 has no return code: a failed call is NaN and the recorded error)
            self._rc(ERR_HIP)
        return v

    def gather(self):
        return self._rc(self.lib.dll.aprilsam_amd_shard_gather_states(self._g, self._p))

    def end(self):
        self.lib.dll.aprilsam_amd_shard_end(self._p)

    def snapshot(self):
        return dict(states=self.g.states(), lp=self.g.l_points(), dx=self.g.deltas())

    def close(self):
        self.p.destroy(); self.g.destroy()


def standard_run(R, iters=1):
    """begin / comm_init_host / chi2 / iterate x iters / chi2 / gather_states / shard_info 0-3 / end on one rank -> dict"""
    out = dict(rank=R.rank, rc_begin=R.begin())
    if out["rc_begin"] != 0:
        return out
    out["info"] = [R.info(w) for w in range(4)]
    out["chi2"] = [R.chi2()]
    out["rc_iterate"] = []
    for _ in range(iters):
        out["rc_iterate"].append(R.iterate(1))
        out["chi2"].append(R.chi2())
    out["rc_gather"] = R.gather()
    out["stats"] = R.p.stats()
    out.update(R.snapshot())
    R.end()
    return out


def run(lib, arrays, world, body=standard_run, timeout=TIMEOUT, **kw):
    """`body(Rank, **kw)` on every rank of a `world`-rank run of the graph `arrays` -> (per-rank results, fabric)"""
    assert_usable()
    bind(lib)
    fabric = Fabric(world, timeout)
    start = threading.Barrier(world)

    def one(rank):
        R = Rank(lib, fabric, rank, arrays)
        try:
            start.wait(TIMEOUT)
            return body(R, **kw)
        finally:
            R.end(); R.close()
    res = run_threads(world, one)
    assert_usable()
    return res, fabric


def expected_log(rank, world, xfer, bcast, n_levels, n_nodes, iters=1):
    """what standard_run makes the library call on `rank`, from aprilsam_amd_shard_info 1 (xfer: level, front, src, dst, -, count) and 2
    (bcast: level, front, owner, first, nsb): chi2 = one 1-double all-reduce; an iteration = per level, in list order, this rank's sends
    and receives of the packed counts, then per level from the top one broadcast of 3 nsb doubles per top front on EVERY rank, then the
    1-double all-reduce of the pivot flag; the gather = one all-reduce of 9 N doubles.  world = 1 has no transport: nothing."""
    if world == 1:
        return []
    xfer = np.asarray(xfer).reshape(-1, 6); bcast = np.asarray(bcast).reshape(-1, 5)
    it = []
    for l in range(n_levels):
        for lev, front, src, dst, _, cnt in xfer[xfer[:, 0] == l]:
            if src == rank:
                it.append(("send", int(cnt), int(dst)))
            elif dst == rank:
                it.append(("recv", int(cnt), int(src)))
    for l in range(n_levels - 1, -1, -1):
        for lev, front, own, first, nsb in bcast[bcast[:, 0] == l]:
            it.append(("bcast", 3 * int(nsb), int(own)))
    it.append(("allreduce", 1, -1))
    chi2 = [("allreduce", 1, -1)]
    return chi2 + iters * (it + chi2) + [("allreduce", 9 * int(n_nodes), -1)]
