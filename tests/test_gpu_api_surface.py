"""The small print of the reference API, on the GPU, against the live reference where it has a defined behaviour:

* april_graph_cholesky_inc_solver called directly (aprilsam.c:578-597, solve_node's visit rule :721-779);
* the wall-clock fall-back rule (aprilsam.c:557-559) with `batch_time` injected so that it fires deterministically;
* param->delta_x, kept only when the caller pre-allocated it (aprilsam.c:363-366, 590-595);
* param->show_timing (aprilsam.c:316-318, 552-554);
* incremental factors between two OLD poses: identical to the reference where the reference solves its own system,
  and the one class where it does not (different branches of its elimination tree, aprilsam.c:850-906) measured on
  both libraries against the exact solve;
* the failure path (errors.h): out of memory, malformed graphs, unsupported nodes -- no abort, states untouched;
* options changed on a param with a cached plan; factors edited in place on a growing graph.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from aprilsam_amd import datasets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    c, s = np.cos(a[2]), np.sin(a[2]); dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, b[2] - a[2]])


class Walk:
    """a seeded random walk with loop closures, replayed identically on any library exporting the reference API"""

    def __init__(self, lib, seed, nthreshold=10 ** 6, delta=0.05):
        self.rng = np.random.default_rng(seed)
        self.g = lib.new_graph(); self.p = lib.new_param(nthreshold=nthreshold, delta_xy=delta, delta_theta=delta)
        self.truth = [np.zeros(3)]
        self.g.add_node_xyt(self.truth[0]); self.g.add_factor_xytpos(0, [0, 0, 0], datasets.PRIOR_W)
        self.g.cholesky(self.p)

    def info(self):
        M = self.rng.normal(size=(3, 3)); Wk = M @ M.T + np.diag([40.0, 40.0, 120.0]); return (Wk + Wk.T) / 2

    def grow(self, closures=True):
        rng, truth, g = self.rng, self.truth, self.g
        last = truth[-1]
        new = np.array([last[0] + np.cos(last[2]) * 0.8, last[1] + np.sin(last[2]) * 0.8, last[2] + rng.uniform(-0.6, 0.6)])
        truth.append(new); n = len(truth) - 1
        g.add_node_xyt(new + rng.normal(0, [0.15, 0.15, 0.04]))
        g.add_factor_xyt(n - 1, n, _rel(truth[n - 1], new) + rng.normal(0, [0.03, 0.03, 0.01]), self.info())
        if closures and n > 4 and rng.random() < 0.6:
            o = int(rng.integers(0, n - 1))
            g.add_factor_xyt(o, n, _rel(truth[o], truth[n]) + rng.normal(0, [0.03, 0.03, 0.01]), self.info())

    def inc(self, batch_time=1e300):
        self.p.c.batch_time = batch_time
        self.g.cholesky_inc(self.p)

    def snap(self):
        return self.g.chi2(), self.g.states(), self.g.deltas()

    def close(self):
        self.p.destroy(); self.g.destroy()


def _same(a, b, tol=1e-6, what=""):
    (c1, s1, d1), (c2, s2, d2) = a, b
    assert abs(c1 - c2) <= tol * max(abs(c2), 1.0), (what, c1, c2)
    assert np.max(np.abs(s1 - s2)) < tol, (what, float(np.max(np.abs(s1 - s2))))
    assert np.max(np.abs(d1 - d2)) < tol, (what, "delta_X", float(np.max(np.abs(d1 - d2))))


def test_inc_solver_called_directly_matches_the_live_reference(lib, reflib):
    """april_graph_cholesky_inc_solver on its own: right after a batch step (only the root is reached, nothing is updated),
    after an incremental step that marked more than 5 poses (whole tree: every pose gets state = ITS CURRENT l_point + x,
    so l_points moved by the caller in between show up in the states) and after one that marked at most 5 (root only)."""
    runs = []
    for L in (lib, reflib):
        w = Walk(L, 11)
        tr = []
        for _ in range(30):
            w.grow(); w.inc()
        w.g.cholesky(w.p)                               # a batch step, then the solver alone
        w.g.cholesky_inc_solver(w.p); tr.append(w.snap())
        many = few = 0
        for step in range(40):
            w.grow(closures=step % 3 == 0); w.inc()
            before = w.g.states()
            # the caller moves a few linearisation points between the two calls (relinearisation is the harness's business,
            # examples/aprilsam_demo.c:183,190); the solver call must use them
            for i in (1, 7, w.g.n_nodes - 2):
                nd = w.g.node(i)
                nd.l_point[0] += 0.01 * (step + 1); nd.l_point[2] -= 0.002
            w.g.cholesky_inc_solver(w.p)
            tr.append(w.snap())
            moved = np.max(np.abs(w.g.states() - before))
            many += moved > 1e-3; few += moved <= 1e-3
        assert many >= 3 and few >= 3, (many, few)      # both branches of the visit rule were exercised
        runs.append(tr)
        w.close()
    for k, (a, b) in enumerate(zip(*runs)):
        _same(a, b, what=f"step {k}")


def test_wall_clock_rule_follows_the_reference_when_batch_time_is_injected(lib, reflib):
    """aprilsam.c:557-559: `if (step_ms > batch_time / 3) start_over = INT_MAX` -> batch fall-back (:566-575).  The rule is ON by
    default (option deterministic = 0), as in the reference.  batch_time = -1 before a call makes it fire whatever the clock
    says, 1e300 keeps it quiet; a fall-back shows as a rewritten batch_time (:569-572).
      * relinearisation thresholds out of reach: the rule alone decides -> a fall-back exactly at the injected steps;
      * realistic thresholds: the reference sets INT_MAX BEFORE its solver call, whose walk adds one per pose that newly
        crossed the threshold (:741-747) -- the counter wraps negative and the fall-back does NOT happen.  Reproduced as is:
        the same schedule on both libraries gives the same fall-backs and the same states.
    With deterministic = 1 this library ignores the rule."""
    sched = [(-1.0 if k % 5 == 2 else 1e300) for k in range(45)]
    for delta, expect_all in ((50.0, True), (0.05, False)):
        runs, fell = [], []
        for L in (lib, reflib):
            w = Walk(L, 23, delta=delta)
            tr, fb = [], []
            for bt in sched:
                w.grow(); w.inc(bt)
                fb.append(w.p.c.batch_time != bt)
                tr.append(w.snap())
            runs.append(tr); fell.append(fb)
            w.close()
        assert fell[0] == fell[1], (delta, fell)
        fired = [bt < 0 for bt in sched]
        if expect_all:
            assert fell[1] == fired
        else:
            assert not any(f and not r for f, r in zip(fell[1], fired))           # never without the rule (nthreshold is out of reach)
            assert sum(fell[1]) < sum(fired)                                     # the wrap swallowed some of them
        for k, (a, b) in enumerate(zip(*runs)):
            _same(a, b, what=f"delta {delta} step {k}")
    lib.set_option("deterministic", 1)
    try:
        w = Walk(lib, 23, delta=50.0)
        for bt in sched[:12]:
            w.grow(); w.inc(bt)
            assert w.p.c.batch_time == bt                # no fall-back, nothing rewrote it
        w.close()
    finally:
        lib.set_option("deterministic", 0)


def _dx_by_node(w):
    """param->delta_x is laid out like the unknowns, 3 * position in param->ordering (aprilsam.c:141-148, 393-396)"""
    n = w.g.n_nodes
    p = w.p.c
    assert p.nreordering == n
    out = np.zeros((n, 3))
    for pos in range(n):
        out[p.ordering[pos]] = [p.delta_x[3 * pos + k] for k in range(3)]
    return out


def test_delta_x_is_kept_only_when_the_caller_preallocated_it(lib, reflib):
    """aprilsam.c:590-595: x of the step replaces a pre-allocated param->delta_x (fresh zero vector per call, :583: poses the
    walk did not reach read 0); it stays NULL otherwise.  Compared per NODE (the two libraries order the unknowns differently).
    (The batch call's delta_x is left out: the reference stores a pointer it has just freed, aprilsam.c:361-366.)"""
    libc = C.CDLL(None); libc.malloc.restype = C.c_void_p
    runs = []
    for L in (lib, reflib):
        w = Walk(L, 31)
        for _ in range(25):
            w.grow(); w.inc()
        assert not w.p.c.delta_x                            # never allocated by the library on its own
        w.p.c.delta_x = C.cast(libc.malloc(8), C.POINTER(C.c_double))
        tr = []
        for step in range(20):
            w.grow(closures=step % 2 == 0); w.inc()
            tr.append((_dx_by_node(w), w.g.deltas()))
        runs.append(tr)
        w.close()                                           # (param_destory frees delta_x on both sides)
    nz = 0
    for k, ((x1, d1), (x2, d2)) in enumerate(zip(*runs)):
        assert np.max(np.abs(x1 - x2)) < 1e-6, k
        assert np.max(np.abs(d1 - d2)) < 1e-6, k
        touched = np.any(x2 != 0, axis=1)
        assert np.allclose(x2[touched], d2[touched], atol=0)          # where the walk went, delta_x == the node's delta_X
        nz += int(touched.sum() < len(touched))
    assert nz > 0                                           # some steps only walked the marked root paths: zeros elsewhere


def test_show_timing_prints_a_line_per_call(lib, capfd):
    """aprilsam.c:316-318, 552-554: param->show_timing makes every solver call print its time profile"""
    w = Walk(lib, 5)
    w.p.c.show_timing = 1
    w.grow(); w.inc()
    w.g.cholesky(w.p)
    w.g.cholesky_inc_solver(w.p)
    w.p.c.show_timing = 0
    w.grow(); w.inc()
    out = capfd.readouterr().out
    assert out.count("aprilsam_amd inc:") == 1 and out.count("aprilsam_amd batch:") == 1 and out.count("aprilsam_amd solve:") == 1
    w.close()


# ---- factors between two OLD poses -----------------------------------------------------------------------------------------
def _old_old_case(L, oracle, seed, a, b, nbase=40):
    """batch on a random graph, then ONE incremental call that adds a single factor between the old poses a and b.
    Returns (states after, exact solution of the incremental system at the l_points, states before)"""
    st, fa, fb, z, W = datasets.random_pose_graph(nbase, 12, seed)
    g = L.new_graph(); g.build_from_arrays(st, fa, fb, z, W); p = L.new_param(nthreshold=10 ** 6)
    g.cholesky(p)
    lp = g.l_points(); before = g.states()
    rng = np.random.default_rng(seed + 1000)
    zz = _rel(st[a], st[b]) + rng.normal(0, [0.05, 0.05, 0.02]); Wk = np.diag([50.0, 50.0, 200.0]).reshape(9)
    g.add_factor_xyt(a, b, zz, Wk)
    p.c.batch_time = 1e300
    g.cholesky_inc(p)
    after = g.states()
    flags = p.stats() if L.is_product else None           # (what the caller is told: stats.inc_old_old_cross / inc_replanned)
    fa2 = np.append(fa, a).astype(np.int32); fb2 = np.append(fb, b).astype(np.int32)
    dx = oracle.solve_system(lp, lp, fa2, fb2, np.vstack([z, zz]), np.vstack([W.reshape(-1, 9), Wk]), np.full(len(st), 1e-4))
    exact = lp + dx; exact[:, 2] = [oracle.mod2pi(v) for v in exact[:, 2]]
    p.destroy(); g.destroy()
    return (after, exact, before, flags) if flags is not None else (after, exact, before)


def test_factors_between_two_old_poses_against_the_live_reference(lib, reflib, oracle):
    """A new factor whose two poses both predate the call -- unreachable from the reference's own harnesses (the demo copies a
    factor when its LATER pose arrives, examples/aprilsam_demo.c:150-163; the tutorial's only loop closure involves the
    newest pose, examples/aprilsam_tutorial.c:241-258) but legal through the API.  Two classes, told apart by the reference's
    own result:
      * the reference solves its own system (one pose is an ancestor of the other in its elimination tree): this library
        returns the same states to 1e-6 -- the case is part of the live-reference comparison;
      * the two poses sit in different branches: the reference's partial re-factorisation walks the OLD tree children first
        (aprilsam.c:850-906) and finalises one row before the other has updated it; its result is NOT the solution of its own
        normal equations.  This library re-plans and returns the exact solve; both distances to the exact solution are
        measured here on the same inputs and pinned (ours <= 1e-8, the reference's > 1e-4), so the deviation is a number in
        the test log, not an anecdote."""
    same_branch = cross = 0
    worst_ref = worst_ours = 0.0
    for seed in range(14):
        rng = np.random.default_rng(seed)
        a, b = sorted(rng.choice(np.arange(1, 39), 2, replace=False).tolist())
        ours, exact, before, flags = _old_old_case(lib, oracle, seed, a, b)
        ref, exact2, _ = _old_old_case(reflib, oracle, seed, a, b)
        assert np.max(np.abs(exact - exact2)) < 1e-12
        touched = np.any(ref != before, axis=1)          # the poses the reference's walk updated
        assert touched.any()
        d_ref = float(np.max(np.abs(ref[touched] - exact[touched])))
        d_ours = float(np.max(np.abs(ours[touched] - exact[touched])))
        assert np.array_equal(np.any(ours != before, axis=1), touched), seed       # same poses written on both sides
        assert d_ours < 1e-8, (seed, d_ours)
        if d_ref < 1e-8:
            same_branch += 1
            assert np.max(np.abs(ours - ref)) < 1e-6, seed
            assert flags["inc_old_old_cross"] == 0, (seed, flags)
        else:
            cross += 1
            # the deviation is REPORTED: the caller reads from the stats that this step's states are the exact solve, not the
            # reference's (include/aprilsam_amd.h)
            assert flags["inc_old_old_cross"] == 1 and flags["inc_replanned"] == 1, (seed, flags)
            worst_ref = max(worst_ref, d_ref); worst_ours = max(worst_ours, d_ours)
    print(f"old-old factors: {same_branch} cases where the reference is exact (identical here), {cross} cross-branch cases: "
          f"max distance to the exact solve  reference {worst_ref:.3e}  this library {worst_ours:.3e}")
    assert same_branch >= 2 and cross >= 2
    assert worst_ref > 1e-4 and worst_ours < 1e-8


def test_a_nan_delta_skips_that_pose_on_the_device_as_the_reference_does(lib, reflib):
    """april_graph_xyt.c:304-305: a node whose dx holds a NaN is skipped by update() -- state AND delta_X stay.  Driven through the
    DEVICE guards here (the state update that rides on the back substitution, kernels.hip.h backsolve_finish, and
    k_update_states), not through the host vtable: a pose of its own connected component whose only factor is a prior with a
    NaN in z gets dx = NaN from the solve, everything else is unaffected.  Both the API call (host objects in/out) and the
    resident loop (states never leave HBM between the iterations: only the device guard can protect the pose) against the
    live reference."""
    st, fa, fb, z, W = datasets.random_pose_graph(40, 14, 5)
    lone = len(st)                                           # one more pose, connected to nothing ...
    st = np.vstack([st, [3.0, -2.0, 0.4]])
    fa = np.append(fa, lone).astype(np.int32); fb = np.append(fb, -1).astype(np.int32)
    z = np.vstack([z, [np.nan, 0.5, 0.1]]); W = np.vstack([W.reshape(-1, 9), np.diag([10.0, 10.0, 10.0]).reshape(1, 9)])   # ... but to a prior with a NaN
    out = {}
    for name, L in (("ours", lib), ("ref", reflib)):
        g = L.new_graph(); g.build_from_arrays(st, fa, fb, z, W); p = L.new_param()
        d0 = g.deltas().copy()
        for _ in range(3):
            g.cholesky(p)
        out[name] = (g.states().copy(), g.deltas().copy(), d0)
        p.destroy(); g.destroy()
    so, do, d0 = out["ours"]; sr, dr, _ = out["ref"]
    assert np.array_equal(sr[lone], st[lone]) and np.array_equal(dr[lone], d0[lone])          # the reference skipped the pose ...
    assert np.array_equal(so[lone], st[lone]) and np.array_equal(do[lone], d0[lone])          # ... and so did this library
    assert not np.isnan(so).any() and np.max(np.abs(so - sr)) < 1e-6 and np.max(np.abs(do[:lone] - dr[:lone])) < 1e-6
    assert np.max(np.abs(so[:lone] - st[:lone])) > 1e-3                                       # (the others did move)
    # resident loop: three iterations on the device, states written back once at the end
    g = lib.new_graph(); g.build_from_arrays(st, fa, fb, z, W); p = lib.new_param()
    g.batch_resident(p, 3)
    s3 = g.states()
    assert np.array_equal(s3[lone], st[lone]) and not np.isnan(s3).any()
    assert np.max(np.abs(s3 - sr)) < 1e-6
    assert p.stats()["not_spd"] == 0
    p.destroy(); g.destroy()


def test_tail_poses_changed_between_two_incremental_steps_forces_a_replan(lib, reflib):
    """the frozen base + tail plan of the incremental path bakes in option tail_poses (the padded shape of the last
    tail front).  Raising it between two april_graph_cholesky_inc calls must not drive the old layout with the new value: the
    step re-plans (stats.inc_replanned) and the run stays on the live reference's states."""
    try:
        runs = []
        for L in (lib, reflib):
            w = Walk(L, 23)
            snaps = []
            for k in range(60):
                w.grow()
                if L.is_product and k == 20:
                    lib.set_option("tail_poses", 40)
                w.inc()
                if L.is_product and k == 20:
                    assert w.p.stats()["inc_replanned"] == 1
                if L.is_product and k == 22:
                    assert w.p.stats()["inc_replanned"] == 0
                snaps.append(w.snap())
            runs.append(snaps); w.close()
        for k, (a, b) in enumerate(zip(*runs)):
            _same(a, b, 1e-6, f"step {k}")
    finally:
        lib.set_option("tail_poses", 28)


# ---- failure path --------------------------------------------------------------------------------------------------------
def test_out_of_memory_returns_cleanly_and_the_next_call_works(lib):
    """errors.h: a refused device allocation (option mem_cap_mb stands in for a full device) ends the call with the node
    states untouched, error -11 in stats / aprilsam_amd_last_error, no abort; once memory is there the same param works"""
    arr = lib.lattice_arrays(60)
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    before = g.states().copy()
    lib.clear_error()
    lib.set_option("mem_cap_mb", 1)
    try:
        g.cholesky(p)
    finally:
        lib.set_option("mem_cap_mb", 0)
    code, msg = lib.last_error()
    assert code == -11 and "mem_cap_mb" in msg
    assert p.stats()["error_code"] == -11
    assert np.array_equal(g.states(), before) and np.isnan(g.deltas()).sum() == 0
    p.c.batch_time = 1e300
    g.cholesky_inc(p)                                    # no factorisation to extend: silent return (aprilsam.c:382-383)
    assert np.array_equal(g.states(), before)
    from tests.conftest import golden
    G = golden("lattice_60.npz")
    chi2 = [g.chi2()]
    for _ in range(len(G["chi2"]) - 1):
        g.cholesky(p); chi2.append(g.chi2())
    assert p.stats()["error_code"] == 0
    assert np.max(np.abs(np.array(chi2) - G["chi2"]) / G["chi2"]) < 1e-8
    p.destroy(); g.destroy()


def test_malformed_and_unsupported_graphs_are_refused_without_abort(lib):
    arr = datasets.random_pose_graph(30, 10, 4)
    # a factor connecting a node to itself
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.add_factor_xyt(3, 3, [0, 0, 0], np.eye(3))
    before = g.states().copy()
    g.cholesky(p)
    assert lib.last_error()[0] == -13 and "itself" in lib.last_error()[1] and np.array_equal(g.states(), before)
    assert np.isnan(g.chi2())                            # chi^2 cannot be evaluated either: NaN, not a crash
    p.destroy(); g.destroy()
    # a node index out of range
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.add_factor_xyt(2, 31, [0, 0, 0], np.eye(3))
    g.cholesky(p)
    assert lib.last_error()[0] == -13 and np.array_equal(g.states(), before)
    p.destroy(); g.destroy()
    # a node type other than xyt (aprilsam.h:94)
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.node(5).type = 77
    g.cholesky(p)
    assert lib.last_error()[0] == -12 and np.array_equal(g.states(), before)
    g.node(5).type = 100
    g.cholesky(p)                                        # and the same objects work once the graph is legal
    assert p.stats()["error_code"] == 0 and not np.array_equal(g.states(), before)
    # nreordering == 0: the reference asserts (aprilsam.c:372-374)
    st = g.states().copy()
    p.c.nreordering = 0
    g.cholesky(p)
    assert lib.last_error()[0] == -12 and np.array_equal(g.states(), st)
    p.destroy(); g.destroy()
    lib.clear_error()
    assert lib.last_error() == (0, "")


# ---- plan cache vs options / edits ----------------------------------------------------------------------------------------
def test_options_changed_on_a_param_with_a_cached_plan_force_a_replan(lib, oracle):
    """launch tables are built for the options in force at plan time and read again at enqueue time: toggling
    blk_backsolve / syrk_small_tiles / small_lds_kb on a warm param (no graph replay, so the live enqueue code runs) must re-plan"""
    arr = lib.lattice_arrays(40)
    oc, ost = oracle.iterate(arr, 1)
    lib.set_option("use_graph", 0); lib.set_option("small_lds_kb", 0)
    try:
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        st0 = g.states().copy()
        for name, val in (("blk_backsolve", 0), ("syrk_small_tiles", 0), ("syrk_xcd_order", 1), ("small_lds_kb", 64), ("syrk_small_tiles", 320), ("blk_backsolve", 1), ("syrk_xcd_order", 512)):
            g.cholesky(p)
            assert p.stats()["not_spd"] == 0 and np.max(np.abs(g.states() - ost)) < 1e-6, name
            for i in range(g.n_nodes):
                g.set_state(i, st0[i])
            lib.set_option(name, val)
            g.cholesky(p)
            assert p.stats()["symbolic_reused"] == 0, name
            assert p.stats()["not_spd"] == 0 and np.max(np.abs(g.states() - ost)) < 1e-6, name
            for i in range(g.n_nodes):
                g.set_state(i, st0[i])
        p.destroy(); g.destroy()
    finally:
        for name, val in (("use_graph", 1), ("small_lds_kb", 156), ("blk_backsolve", 1), ("syrk_small_tiles", 320), ("syrk_xcd_order", 512)):
            lib.set_option(name, val)


def test_factor_edited_in_place_on_a_growing_graph_matches_the_live_reference(lib, reflib):
    """the batch call on a graph that grew since the plan was made keeps the plan (batch_extend); z / W of OLD factors edited
    in place before that call must still reach the device (the reference re-reads every factor, aprilsam.c:152-190)"""
    out = []
    for L in (lib, reflib):
        w = Walk(L, 41)
        tr = []
        for step in range(30):
            w.grow()
            if step % 4 == 1:
                f = w.g.factor(1 + step // 2)
                f.u.z[0] += 0.05; f.u.z[2] -= 0.01
                f.u.W.contents.data[0] *= 1.5
            w.g.cholesky(w.p)
            tr.append(w.snap())
        out.append(tr)
        w.close()
    for k, (a, b) in enumerate(zip(*out)):
        _same(a, b, what=f"step {k}")


# ---- the runtime's lazy initialisations: at april_graph_cholesky_param_init, not inside the first solver calls ----------------
def _first_call(env_extra):
    env = dict(os.environ); env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "first_call.py"), "--chi2"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    ms = {}; chi2 = None
    for ln in r.stdout.splitlines():
        if ln.startswith("first april_graph_cholesky (1 pose):"): ms["tiny"] = float(ln.split(":")[1].split()[0])
        if ln.startswith("first call on M3500"): ms["m3500"] = float(ln.split(":")[1].split()[0])
        if ln.startswith("chi2 after two M3500 calls:"): chi2 = ln.split(":")[1].strip()
    assert "tiny" in ms and "m3500" in ms and chi2 is not None, r.stdout
    return ms, chi2


def test_warm_up_moves_the_lazy_initialisations_out_of_the_first_solver_calls(built):
    """option warm_up (solver.hip.cpp: warm_up): with it the first call of a fresh process is a solver call, not 20 ms of stream /
    copy-engine / code-object set-up; without it (APRILSAM_AMD_WARM_UP=0) everything stays lazy; the results are the same bits"""
    warm, chi_w = _first_call({})
    lazy, chi_l = _first_call({"APRILSAM_AMD_WARM_UP": "0"})
    assert chi_w == chi_l, (chi_w, chi_l)
    assert warm["tiny"] < 0.5 * lazy["tiny"], (warm, lazy)          # measured 0.5 against 24 ms
    assert warm["tiny"] < 8.0, warm


def test_a_graph_per_solve_recycles_its_stream_and_gives_the_same_bits(lib):
    """solver_pack.inc.h: take_stream / park_stream -- a released graph parks its stream, the next graph of the slot takes it"""
    arr = datasets.m3500_batch()
    ref = None
    for k in range(6):
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        g.cholesky(p); g.cholesky(p)
        st = g.states().copy(); c = g.chi2()
        if ref is None: ref = (st, c)
        else: assert np.array_equal(st, ref[0]) and c == ref[1], k
        p.destroy(); g.destroy()


def test_chi2_of_a_large_graph_sums_in_two_stages_reproducibly(lib):
    """april_graph_chi2 above 65 536 factors (kernels.hip.h: k_reduce_parts + k_reduce): the 100 k lattice's 397 531 terms -- the same bits on
    every call, the unmodified reference's value (bench.LATTICE100K_CHI2, golden of oracle/_ref) to rounding; below the limit the one-stage sum"""
    import bench
    g = lib.new_graph(); nfac = lib.dll.aprilsam_amd_make_lattice(g.ptr, 316)
    assert nfac == 397531
    c = [g.chi2() for _ in range(4)]
    assert c[0] == c[1] == c[2] == c[3]
    assert abs(c[0] - bench.LATTICE100K_CHI2[0]) / bench.LATTICE100K_CHI2[0] < 1e-13
    g.destroy()
    g = lib.new_graph(); assert lib.dll.aprilsam_amd_make_lattice(g.ptr, 100) < 65536
    c = [g.chi2() for _ in range(3)]
    assert c[0] == c[1] == c[2] and c[0] > 0
    g.destroy()


# ---- bench.py --gpus 2, before the 8-GPU node meets it ---------------------------------------------------------------------
def test_bench_two_ranks_on_one_gpu_prints_one_valid_line(built):
    """the driver's multi-GPU command line, with the two ranks sharing cuda:0 and gloo instead of RCCL (two ranks cannot share
    a device under RCCL): torch.distributed.run plumbing, replica timing, the sharded config-5 branch on a small lattice"""
    import json
    port = 29500 + os.getpid() % 400
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--one-gpu", "--full",
           "--backend", "gloo", "--lattice1m-k", "316", "--no-cpu-baseline", "--no-inc"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    from tests.support.bench_line import check_line
    out = check_line(r.stdout.splitlines()[-1], cpu_baseline=False)          # the LAST stdout line is what the driver parses
    assert out["n_gpus"] == 2 and out["steps"] == 5 and out["scaling"] == "weak" and out["value"] > 0
    assert out["unit"] == "GN iterations/s" and out["roofline"]["frac"] > 0
    cfg = out["config"]
    assert "lattice1m_error" not in cfg, cfg
    assert cfg["lattice1m_n_gpus"] == 2 and cfg["lattice1m_ms_per_step"] > 0 and cfg["lattice1m_chi2_relerr_max"] < 1e-9
    assert cfg["lattice1m_transport"].startswith("host callbacks") and cfg["lattice1m_comm_bytes_per_iteration"] > 0
    # the nested record went to the side file
    ex = json.load(open(os.path.join(ROOT, out["extras"])))
    l1 = ex["lattice1m"]
    assert l1["n_gpus"] == 2 and "shards x2" in l1["parallelism"]
    assert max(l1["chi2_relerr_vs_reference"]) < 1e-9
    assert ex["multi_gpu"]["world"] == 2 and ex["multi_gpu"]["transport"].startswith("host callbacks")


def test_bench_plain_run_prints_the_headline_and_dumps_what_the_steps_left(built, tmp_path):
    """bench.py without --full: the contract fields of the timed steps only, and --dump-outputs writes the node objects they left --
    after 6 warm-up + 4 timed steps, the states of the reference's 10 batch iterations (golden)"""
    import json
    from tests.conftest import golden
    d = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "6", "--dump-outputs", str(d)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.splitlines()[-1])
    assert out["steps"] == 4 and out["warmup"] == 6 and out["n_gpus"] == 1
    assert out["unit"] == "GN iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-4)
    assert not any(k in out for k in ("roofline", "cpu_baseline", "value_api_call", "extras"))
    arrs = {k: np.load(d / f"{k}.npy") for k in ("states", "l_points", "deltas")}
    for a in arrs.values():
        assert a.dtype == np.float64 and a.shape == (3500, 3) and np.all(np.isfinite(a))
    assert np.max(np.abs(arrs["states"] - golden("m3500_batch.npz")["final_states"])) < 1e-6
