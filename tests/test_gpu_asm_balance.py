"""The extend-add behind the wait (kernels.hip.h: assemble_front) with the plan's column owners (option asm_balance, plan.h: asm_owners) against
column mod waves.  One wave per destination column either way, adding child after child, so every sum keeps its order: states, deltas and
l_points must be bitwise equal after three resident steps -- on every workgroup width (the table is built for the width of the front's launch;
another width, multi-workgroup fronts and the fronts the incremental path regenerates fall back to the modulo rule), level by level, with no
front in LDS, and with every hand-over poisoned first.  The first step's dx is also compared with the numpy emulation of the device algorithm
(tests/support/mf_emulator.py) at the tolerance of tests/test_gpu_stages.py, rtol 1e-12 / atol 1e-9 (measured: at most 4.2e-10 on M3500 with
|dx| up to 31, 2.4e-11 elsewhere).  Owners 0 and 1 share the LDS adds (no-return atomics) and the pass over children with more than 128 rows,
which now runs only where a work list holds such a block -- the lattices do (asserted from the plan), M3500 does not -- so the bitwise
comparison cannot see an error in either: the emulation is their independent check.

That the device reads the owner table at all -- the bitwise comparison would pass with every front on the modulo rule -- is shown by the
length of wave 0's work list, which the debug stamps keep per front: the table's on M3500 with asm_balance 1, the modulo rule's with 0.

More than CAPQ = 64 children: a star's hub front has one child per leaf domain -- the 1200-leaf star's plan is asserted to have such a front."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets, harness
from tests.support.mf_emulator import PlanView, contributions, solve
import tests.test_gpu_parity as T
from tests.test_asm_balance import _lists, _owners
from tests.test_gpu_persist_leaves import _same, resident3

pytestmark = pytest.mark.gpu
CAPQ = 64
OPTION_SETS = [{}, {"small_threads": 256}, {"small_threads": 512}, {"persist": 0}, {"small_lds_kb": 0}, {"pool_poison": 1}]
GRAPHS = ["m3500", "chain_300", "random_300", "lattice_40", "lattice_60", "star_1200"]
EMU_RTOL, EMU_ATOL = 1e-12, 1e-9                          # tests/test_gpu_stages.py


def _arr(lib, name):
    return {"m3500": datasets.m3500_batch, "chain_300": lambda: T._chain(300, 3), "random_300": lambda: datasets.random_pose_graph(300, 200, 3),
            "lattice_40": lambda: lib.lattice_arrays(40), "lattice_60": lambda: lib.lattice_arrays(60), "star_1200": lambda: T._star(1200, 5)}[name]()


@pytest.fixture(scope="module")
def cases(lib, oracle):
    """per graph, once: the arrays, the plan, and the emulation's dx of the first Gauss-Newton step (node order)"""
    out = {}
    for name in GRAPHS:
        arr = _arr(lib, name)
        st, fa, fb, z, W = arr
        P = PlanView(lib, len(st), fa, fb, xy=st[:, :2], leaf_nodes=16)
        H, G = contributions(oracle, st, st, fa, fb, z, W, P.factor_swap)
        dx = solve(P, H, G, np.full(len(st), 1e-4)).reshape(len(st), 3)[P.pos]
        out[name] = (arr, P, dx)
    return out


def _tall_blocks(P):
    """child blocks with rows beyond 128 below them: what the extend-add's tail pass is for"""
    return sum(1 for t in range(P.nF) if P.front_parent[t] >= 0 for jb in range(int(P.front_nub[t])) if 3 * int(P.front_nub[t]) + 1 - 3 * jb > 128)


def test_plans_hold_what_the_cases_are_for(cases):
    tall = {name: _tall_blocks(cases[name][1]) for name in GRAPHS}
    most_kids = {name: int(np.max(np.diff(cases[name][1].ch_ptr))) for name in GRAPHS}
    print(f"[asm_balance] child blocks with rows beyond 128: {tall}; most children of one front: {most_kids}")
    assert tall["m3500"] == 0                               # the tail pass has nothing to do on the flagship workload
    assert tall["lattice_40"] > 0 and tall["lattice_60"] > 0      # ... and is kept busy here
    assert most_kids["star_1200"] > CAPQ                   # child records staged in more than one group


@pytest.mark.parametrize("name", GRAPHS)
def test_bitwise_against_the_modulo_rule_and_close_to_the_emulation(lib, cases, name):
    arr, P, dx_emu = cases[name]
    for opts in OPTION_SETS:
        a = resident3(lib, arr, asm_balance=0, **opts)
        b = resident3(lib, arr, asm_balance=1, **opts)
        assert a[4]["error_code"] == 0 and b[4]["error_code"] == 0 and b[4]["not_spd"] == 0, (name, opts, a[4], b[4])
        assert np.isfinite(b[0]).all() and np.isfinite(b[1]).all()
        _same(b, a, (name, opts, "asm_balance 1 against 0"))
        with lib.options(asm_balance=1, **opts):           # (asm_balance 0 has the same bits: just shown)
            _, snaps, stats = T.run_batch(lib, arr, 1)
        err = float(np.max(np.abs(snaps[0][1] - dx_emu)))
        print(f"[asm_balance] {name} {opts}: first step's dx against the emulation {err:.3e} (largest entry {float(np.max(np.abs(dx_emu))):.3e})")
        assert stats["error_code"] == 0 and np.allclose(snaps[0][1], dx_emu, rtol=EMU_RTOL, atol=EMU_ATOL), (name, opts, err)


def test_the_device_reads_the_owner_table(lib, cases, monkeypatch):
    """M3500 with the defaults is one 1024-thread launch of single-workgroup fronts, so every front with children has a table for 16 waves.  The
    debug stamps keep the length of wave 0's first work list per front (slot 7; no M3500 list needs a second fill): with asm_balance 1 it must be
    what aprilsam_amd_asm_owners gives wave 0, with 0 what column mod 16 gives it -- and the two differ, or this would show nothing."""
    monkeypatch.setenv("APRILSAM_AMD_KPROF", "1")          # (read when a plan is uploaded)
    arr, P, _ = cases["m3500"]
    tree = (P.front_parent, P.front_nsb, P.front_nub, P.front_rows_ptr, P.front_rel)
    bal, mod = _lists(*tree, 16, _owners(lib, *tree, 16))
    parents = np.nonzero(np.diff(P.ch_ptr) > 0)[0]
    assert int(np.max(np.diff(P.ch_ptr))) <= CAPQ and max(bal.max(), mod.max()) <= 64      # one group of child records, one fill per list
    assert np.any(bal[parents, 0] != mod[parents, 0])
    for balance, want in ((1, bal), (0, mod)):
        with lib.options(asm_balance=balance, use_graph=0):
            g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
            g.cholesky(p)
            nF = p.stats()["n_fronts"]
            assert nF == P.nF
            buf = np.zeros((nF, 16), np.int64)
            assert lib.dll.aprilsam_amd_debug_front_times(p.ptr, buf.ctypes.data_as(C.POINTER(C.c_longlong)), nF) == nF
            p.destroy(); g.destroy()
        assert np.all(buf[parents, 6] > 0)                 # every parent went through the small fronts' extend-add
        differ = parents[buf[parents, 7] != want[parents, 0]]
        assert len(differ) == 0, (balance, differ[:8], buf[differ[:8], 7], want[differ[:8], 0])


def test_incremental_demo_takes_the_fall_back_with_the_same_bits(lib):
    """first 300 poses of the incremental demo: tail fronts and regenerated fronts have no owner table; the batch fall-back steps have one"""
    res = {}
    for bal in (0, 1):
        with lib.options(asm_balance=bal):
            res[bal] = harness.run_demo(lib, datasets.m3500_arrays(), max_poses=300, deterministic=True)
    assert np.array_equal(res[0]["was_batch"], res[1]["was_batch"]) and res[0]["was_batch"].sum() >= 2
    assert res[0]["final_states"].tobytes() == res[1]["final_states"].tobytes(), float(np.max(np.abs(res[0]["final_states"] - res[1]["final_states"])))
    assert res[0]["chi2"].tobytes() == res[1]["chi2"].tobytes()
