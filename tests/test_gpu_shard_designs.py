"""The sharded solve (csrc/solver_shard.inc.h) on designed trees, rank counts and edge cases: every (graph, world) of
tests/support/shard_designs.py -- idle ranks, ghosts that are their parent's primary child, ghost update blocks at the pass edges of the
extend-add and at k_pack_update's stride, 32 and 35 remote children of one front, several roots, worlds of 3 and 5 ranks, asymmetric W,
M3500 -- as THREADS of this process over tests/support/thread_comm.py (one process holds the GPU; the process-spawning lattice tests of
tests/test_gpu_shard.py stay the only ones on the gloo and RCCL wires).

One Gauss-Newton iteration from the builder's states; on EVERY rank: return codes 0, no failed pivot, no error; the gathered l_points are
the input bit for bit; states, l_points and dx are bit-identical on all ranks; the residual of the normal equations at the l_points is below
the project's bar RES_RTOL (not for asym_batch: tests/support/normal_eq.py); dx within DX_FACTOR x ORDER_DEV of the oracle's (clique trees,
the bound of tests/test_gpu_front_shapes.py), states within 1e-9 of a world = 1 run of the same library (the other symmetric graphs, the bar
of tests/test_gpu_shard.py), states within STATE_ATOL of the reference's golden (asym_batch); aprilsam_amd_shard_chi2 before and after within
1e-9 relative of the oracle's; the log of the transport's callbacks equals the schedule that aprilsam_amd_shard_info 1 and 2 of the same run
describe (thread_comm.expected_log); the pool of every rank has the doubles of its fronts and ghosts, 0 for an idle rank.

Nothing bitwise is asserted between a sharded and a single-rank run (DESIGN.md promises none); the deviation is printed (FIGURE| lines) and
recorded in DESIGN.md section 31, with the two failure contracts at the end of this file and the scratch mutations these tests were seen
to catch."""
import threading
import time

import numpy as np
import pytest

from tests.conftest import golden
from tests.support import clique_trees as CT
from tests.support import pivot_placement as pp
from tests.support import shard_designs as D
from tests.support import thread_comm as TC
from tests.support.normal_eq import normal_equation_residual

pytestmark = pytest.mark.gpu
LAM = 1e-4
RES_RTOL = 1e-10                      # tests/test_gpu_normal_eq.py
DX_FACTOR = 100                       # tests/test_gpu_front_shapes.py
DX_ATOL = DX_FACTOR * CT.ORDER_DEV
SINGLE_ATOL = 1e-9                    # tests/test_gpu_shard.py: sharded against single-rank states
STATE_ATOL = 1e-6                     # tests/test_gpu_asymmetric_w.py, tests/test_gpu_parity.py
CHI2_RTOL = 1e-9
ITER_CHI2_RTOL = 1e-8                 # several iterations against oracle.iterate: the bars of tests/test_gpu_parity.py / test_gpu_slots.py
OPTION_SETS = [dict(small_lds_kb=0), dict(small_lds_kb=0, blk_backsolve=0), dict(wave_backsolve=0), dict(small_threads=256)]
SHORT_TIMEOUT = 2.0                   # seconds: the fabric's timeout once a failure has been injected (the healthy part runs under TC.TIMEOUT)

_REF, _SINGLE, _FIG = {}, {}, {}


def _freeze(*a):
    for x in a:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return a


def _reference(lib, oracle, name, arr=None, key=None):
    """(states after one step, dx, chi2 before, chi2 after) of the oracle -- for asym_batch of the reference's golden; computed once"""
    key = key or name
    if key not in _REF:
        arr = arr if arr is not None else D.arrays(lib, name)
        if name == "asym_batch":
            G = golden("asym_batch.npz")
            assert all(np.array_equal(a, b) for a, b in zip(arr, (G["states"], G["fa"], G["fb"], G["z"], G["W"])))
            _REF[key] = _freeze(np.array(G["states_after"][0]), np.array(G["dx"][0]), float(G["chi2"][0]), float(G["chi2"][1]))
        else:
            st, dx, _ = oracle.batch_step(*arr, lam=LAM)
            _REF[key] = _freeze(st, dx, oracle.chi2(*arr), oracle.chi2(st, *arr[1:]))
    return _REF[key]


def _single(lib, name):
    """a world = 1 run of the same library under the default options (no transport), once per graph"""
    if name not in _SINGLE:
        res, _ = TC.run(lib, D.arrays(lib, name), 1)
        assert res[0]["rc_begin"] == 0 and res[0]["rc_iterate"] == [0] and res[0]["rc_gather"] == 0
        _SINGLE[name] = _freeze(res[0]["states"], res[0]["dx"])
    return _SINGLE[name]


def _figure(key, **vals):
    f = _FIG.setdefault(key, {})
    for k, v in vals.items():
        if not k.startswith("_") and v is not None and (k not in f or v > f[k][0]):
            f[k] = (v, vals.get("_on"))


def _check_schedule(lib, name, arr, world, res, fabric, iters, plan=None):
    """checks 7 and 8, and the run's own plan against the one the design table was declared on"""
    P = plan if plan is not None else D.plan(lib, name)
    M = D.Map(P, world) if world in P.shard else None
    for r, out in enumerate(res):
        nlev, nF, N, pool, pool_all = (int(v) for v in out["info"][0])
        xfer, bcast, owner = out["info"][1].reshape(-1, 6), out["info"][2].reshape(-1, 5), out["info"][3]
        assert (nlev, nF, N) == (P.nLevels, P.nF, len(arr[0])), (name, world, r)
        if M is not None:
            assert np.array_equal(xfer[:, [0, 1, 2, 3, 5]], M.xfer[:, [0, 1, 2, 3, 5]]) and np.array_equal(bcast, M.bcast) and np.array_equal(owner, M.owner), (name, world, r)
            assert pool == M.pool_doubles(r), (name, world, r, pool, M.pool_doubles(r))
            if r not in set(M.owner.tolist()):
                assert pool == 0
        want = TC.expected_log(r, world, xfer, bcast, nlev, N, iters)
        assert fabric.log[r] == want, (name, world, r, len(fabric.log[r]), len(want))
        assert set(fabric.rcs[r]) <= {0}
        assert sum(1 for k in fabric.log[r] if k[0] == "bcast") == iters * len(bcast)


def _check(lib, oracle, name, world, res, fabric, opts, arr=None, ref_key=None, plan=None):
    """checks 1 to 8 of the module docstring on a one-iteration run"""
    arr = arr if arr is not None else D.arrays(lib, name)
    for r, out in enumerate(res):                                                                   # 1
        assert out["rc_begin"] == 0 and out["rc_iterate"] == [0] and out["rc_gather"] == 0, (name, world, r, out.get("rc_begin"), out.get("rc_iterate"), out.get("rc_gather"))
        assert out["stats"]["not_spd"] == 0 and out["stats"]["error_code"] == 0, (name, world, r, out["stats"])
    assert lib.last_error()[0] == 0, lib.last_error()
    for r, out in enumerate(res):
        assert np.array_equal(out["lp"], arr[0]), (name, world, r)                                  # 2
        for k in ("states", "lp", "dx"):                                                            # 3
            assert np.array_equal(out[k], res[0][k]), (name, world, r, k)
        assert out["chi2"] == res[0]["chi2"], (name, world, r)
    st, dx, lp = res[0]["states"], res[0]["dx"], res[0]["lp"]
    want_st, want_dx, c0, c1 = _reference(lib, oracle, name, arr, ref_key)
    resid = dev_dx = dev_single = None
    failures = []
    if name != "asym_batch":                                                                        # 4
        resid = normal_equation_residual(lp, arr[1], arr[2], arr[3], arr[4], dx, LAM)["rel_max"]
        if not resid < RES_RTOL:
            failures.append(("residual", resid))
    if name in D.CLIQUE_GRAPHS:                                                                     # 5
        dev_dx = float(np.max(np.abs(dx - want_dx)))
        if not dev_dx <= DX_ATOL:
            failures.append(("dx against the oracle", dev_dx, DX_ATOL))
    if name == "asym_batch":
        dev_gold = float(np.max(np.abs(st - want_st)))
        if not dev_gold < STATE_ATOL:
            failures.append(("states against the golden", dev_gold))
    bitwise = None
    if ref_key is None:
        s1, d1 = _single(lib, name)
        dev_single = float(np.max(np.abs(st - s1)))
        bitwise = bool(np.array_equal(st, s1) and np.array_equal(dx, d1))
        if name not in D.CLIQUE_GRAPHS and name != "asym_batch" and not dev_single < SINGLE_ATOL:
            failures.append(("states against world = 1", dev_single))
    chi2 = np.array(res[0]["chi2"])                                                                 # 6
    dev_chi2 = float(np.max(np.abs(chi2 - [c0, c1]) / np.array([c0, c1])))
    if not dev_chi2 < CHI2_RTOL:
        failures.append(("chi2", chi2.tolist(), [c0, c1], dev_chi2))
    print(f"FIGURE|{name} @{world}|{opts}|residual {resid}|dx deviation {dev_dx}|sharded vs the default single-rank run {dev_single}|bitwise equal to it {bitwise}|chi2 {dev_chi2:.3e}")
    _figure(str(opts), residual=resid, dx=dev_dx, single=dev_single, chi2=dev_chi2, _on=f"{name} @{world}")
    if bitwise:
        _figure(str(opts), bitwise_cases=1.0, _on=f"{name} @{world}")
    _check_schedule(lib, name, arr, world, res, fabric, 1, plan)                                    # 7, 8
    assert not failures, (name, world, opts, failures)


@pytest.mark.parametrize("entry", D.ALL, ids=D.ident)
def test_designed_entry(lib, oracle, entry):
    name, world = entry
    lib.clear_error()
    res, fabric = TC.run(lib, D.arrays(lib, name), world)
    _check(lib, oracle, name, world, res, fabric, dict())


@pytest.mark.parametrize("entry", D.OPTION_ENTRIES, ids=D.ident)
def test_ghost_readers_and_top_front_solves_in_every_form(lib, oracle, entry):
    """the option sets that change the form of the kernels which read ghosts (k_front_small against k_assemble_big, fewer threads) and which
    back-substitute top fronts (k_backsolve_blk, _t, _w), on every entry with a primary ghost"""
    name, world = entry
    for opts in OPTION_SETS:
        lib.clear_error()
        with lib.options(**opts):                       # (main thread, around the whole run)
            res, fabric = TC.run(lib, D.arrays(lib, name), world)
        _check(lib, oracle, name, world, res, fabric, opts)


@pytest.mark.parametrize("entry", D.THREE_ITERATIONS, ids=D.ident)
def test_three_iterations_against_the_oracle(lib, oracle, entry):
    name, world = entry
    arr = D.arrays(lib, name)
    oc, ost = oracle.iterate(arr, 3, LAM)
    lib.clear_error()
    res, fabric = TC.run(lib, arr, world, iters=3)
    for r, out in enumerate(res):
        assert out["rc_begin"] == 0 and out["rc_iterate"] == [0, 0, 0] and out["rc_gather"] == 0 and out["stats"]["not_spd"] == 0 and out["stats"]["error_code"] == 0
        assert all(np.array_equal(out[k], res[0][k]) for k in ("states", "lp", "dx")) and out["chi2"] == res[0]["chi2"]
    assert lib.last_error()[0] == 0
    dc = float(np.max(np.abs(np.array(res[0]["chi2"]) - oc) / oc)); ds = float(np.max(np.abs(res[0]["states"] - ost)))
    print(f"FIGURE|{name} @{world}|three iterations|chi2 {dc:.3e}|states {ds:.3e}")
    _check_schedule(lib, name, arr, world, res, fabric, 3)
    assert dc < ITER_CHI2_RTOL and ds < STATE_ATOL, (dc, ds)


def test_zz_figures():
    """(prints the maxima over whatever ran before it in this process: DESIGN.md section 31 quotes a run of the whole file)"""
    for key, f in _FIG.items():
        print(f"FIGURE|maxima|{key}|" + "|".join(f"{k} {v[0]:.3e} on {v[1]}" for k, v in f.items()))


# ------------------------------------------------------------------------------------------------------
# the failure contracts
# ------------------------------------------------------------------------------------------------------
def _not_spd_body(R, sync, fabric2, n_factors):
    out = dict(rc_begin=R.begin())
    out["rc"] = R.iterate(1)
    out["stats"] = R.p.stats()
    out["log"] = list(R.fabric.log[R.rank]); out["rcs"] = list(R.fabric.rcs[R.rank])
    out["info"] = [R.info(w) for w in range(4)]
    R.end()
    Wd = R.g.factor(n_factors - 1).u.W.contents.data          # the repair: the knob's information matrix becomes zero
    for k in range(9):
        Wd[k] = 0.0
    sync.wait(TC.TIMEOUT)
    R.fabric = fabric2
    out["again"] = TC.standard_run(R)
    return out


@pytest.mark.parametrize("entry", [("random_300", 3), ("30,25,20 fan 2", 4), ("30,25,20 fan 2", 5)], ids=D.ident)       # (at 5 one rank is idle)
def test_a_failed_pivot_on_the_last_busy_rank_ends_every_rank_with_minus_2(lib, oracle, entry):
    """the indefinite prior of tests/test_gpu_not_spd.py (W = -s e_d e_d', residual 0) on the first pose of a front that the plan gives to the
    last rank that owns anything: the flag all-reduce at the end of shard_iterate makes EVERY rank (the idle ones too) return -2 from the same
    call; after shard_end and the repair a fresh shard_begin on the same objects passes every check of a designed entry"""
    name, world = entry
    base = D.arrays(lib, name)
    P = D.plan(lib, name)
    owner = P.shard[world][2]
    rank = int(owner.max())
    assert rank > 0
    t = int(np.flatnonzero(owner == rank)[0])
    pose = int(P.perm[int(P.front_first[t])])
    arr = pp.with_knob(base, pose, 0, 1e6)
    P2 = D.PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], shard_worlds=(world,))
    assert np.array_equal(P2.shard[world][2], owner) and np.array_equal(P2.perm, P.perm)            # (a prior does not move the plan)
    fabric2, sync = TC.Fabric(world), threading.Barrier(world)
    lib.clear_error()
    res, fabric = TC.run(lib, arr, world, body=_not_spd_body, sync=sync, fabric2=fabric2, n_factors=len(arr[1]))
    for r, out in enumerate(res):
        assert out["rc_begin"] == 0 and out["rc"] == -2, (r, out["rc"])
        assert out["stats"]["not_spd"] == 1, (r, out["stats"])
        xfer, bcast = out["info"][1], out["info"][2]
        want = TC.expected_log(r, world, xfer, bcast, int(out["info"][0][0]), len(arr[0]), 1)[1:-2]       # one iteration, no chi2, no gather
        assert out["log"] == want and out["log"][-1] == ("allreduce", 1, -1) and set(out["rcs"]) == {0}, (r, out["log"][-3:], out["rcs"][-3:])
    repaired = (arr[0], arr[1], arr[2], arr[3], np.vstack([arr[4][:-1], np.zeros((1, 9))]))
    _check(lib, oracle, name, world, [o["again"] for o in res], fabric2, "after the repair", arr=repaired, ref_key=("repaired", name), plan=P2)


def _gather_fails_body(R, sync, fabric2, fail_rank):
    out = dict(rc_begin=R.begin())
    out["rc_iterate"] = R.iterate(1)
    out["chi2_ok"] = R.chi2()
    if R.rank == fail_rank:
        R.fabric.inject.add((fail_rank, "allreduce"))
    sync.wait(TC.TIMEOUT)
    R.fabric.timeout = SHORT_TIMEOUT
    t0 = time.monotonic()
    out["rc_gather"] = R.gather()
    out["t_gather"] = time.monotonic() - t0
    out["chi2_after"] = R.chi2()
    out["log"] = list(R.fabric.log[R.rank]); out["rcs"] = list(R.fabric.rcs[R.rank])
    out["info"] = [R.info(w) for w in range(4)]
    out["nodes"] = R.g.states()
    R.end()
    sync.wait(TC.TIMEOUT)
    R.fabric = fabric2
    out["again"] = TC.standard_run(R)
    return out


def test_a_failing_transport_ends_the_gather_with_minus_6_on_every_rank_and_chi2_is_not_a_partial_sum(lib, oracle):
    """rank 1's callback of the GATHER's all-reduce returns 1 after a clean iteration (nothing is computed on unreceived data): that rank's
    gather_states returns -6 at once, the other ranks' through the fabric's timeout; nobody hangs; aprilsam_amd_shard_chi2 afterwards returns
    NaN, not this rank's partial sum (include/aprilsam_amd.h; before the fix it returned the partial sum); the node
    objects are untouched; after shard_end a fresh run on the same graph and param objects passes every check of a designed entry"""
    name, world, fail_rank = "random_300", 3, 1
    arr = D.arrays(lib, name)
    fabric2, sync = TC.Fabric(world), threading.Barrier(world)
    lib.clear_error()
    res, fabric = TC.run(lib, arr, world, body=_gather_fails_body, sync=sync, fabric2=fabric2, fail_rank=fail_rank)
    c0, c1 = _reference(lib, oracle, name)[2:]
    for r, out in enumerate(res):
        assert out["rc_begin"] == 0 and out["rc_iterate"] == 0 and abs(out["chi2_ok"] - c1) < CHI2_RTOL * c1, (r, out["chi2_ok"], c1)
        assert out["rc_gather"] == -6, (r, out["rc_gather"])
        assert out["t_gather"] < (SHORT_TIMEOUT if r == fail_rank else 3 * SHORT_TIMEOUT), (r, out["t_gather"])
        want = TC.expected_log(r, world, out["info"][1], out["info"][2], int(out["info"][0][0]), len(arr[0]), 1)[1:]          # no chi2 before the iteration
        assert out["log"] == want and out["rcs"] == [0] * (len(want) - 1) + [1], (r, out["log"][-3:], out["rcs"][-3:])
        assert np.array_equal(out["nodes"], arr[0]), r
        print(f"FIGURE|shard_chi2 after a failed transport|rank {r}|{out['chi2_after']!r}|chi2 of the graph {c1!r}")
    again = [o["again"] for o in res]
    for r, out in enumerate(res):
        assert not np.isfinite(out["chi2_after"]), (r, out["chi2_after"], c1)
    code, msg = lib.last_error()                       # (recorded by the chi2 call: the return value has no room for a code)
    assert code == -6 and "aprilsam_amd_shard_chi2" in msg and "transport has failed" in msg, (code, msg)
    lib.clear_error()
    _check(lib, oracle, name, world, again, fabric2, "after a failed transport")
