"""Every incremental step on the GPU against the exact solution of its linear system (tests/support/inc_exact.py): the launch forms of
an incremental step (k_inc_one with tail_refactor or regenerated fronts, low-rank front updates, multi-level and per-level launches, the
inc_tail_solve shortcut, lazy state loads, poisoned hand-overs) on the M3500 demo, the full demo, and the growth scenarios of
tests/test_gpu_parity.py.  Written poses within 1e-9 of l_point + x, visited poses' delta_X within 1e-9 of x, the written / visited
sets those of the reference's bookkeeping, and every batch call and fall-back with a normal-equation residual below 1e-10 -- where the
chi^2-trace tests accept 1e-6 (tests/test_inc_exact.py keeps that gap as a measurement).  Each run prints its figures."""
import pytest

from aprilsam_amd import datasets, harness
from tests.support.inc_exact import IncExact
import tests.test_gpu_parity as T

pytestmark = pytest.mark.gpu
FALLBACKS_700 = [232, 350, 508, 591]
LAUNCH_FORMS = [{"inc_tail": 0}, {"inc_tail": 0, "inc_one": 0}, {"inc_multi": 0}, {"inc_inline": 0}, {"inc_one_spin": 0}, {"inc_one_threads": 1024},
                {"inc_one_threads": 256}, {"inc_one_up": 1, "inc_one_dn": 1}, {"tail_poses": 8}, {"inc_update": 0},
                {"inc_update": 1, "inc_one_up": 16, "inc_one_dn": 16}]
DEMO_OPTIONS = [{}] + LAUNCH_FORMS + [{"inc_fast": 0}, {"inc_tail_solve": 0}, {"inc_lazy_states": 0}, {"inc_replan_tall": 0}, {"pool_poison": 1},
                                      {"pool_poison": 1, "inc_one": 0, "inc_tail": 0}, {"pool_poison": 1, "inc_update": 0, "inc_one": 0}]


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _run(lib, oracle, opts, drive, label, stride=1):
    chk = IncExact(lib, oracle, stride=stride, log=print)
    with lib.options(**opts):
        drive(chk)
    print(f"[inc-exact] {label} {_ids(opts)}: {chk.summary()}")
    r = chk.report
    assert r["failures"] == 0 and r["inc"] > 0 and r["checked"] > 0
    return r


@pytest.mark.parametrize("opts", DEMO_OPTIONS, ids=_ids)
def test_demo_every_step_is_the_exact_solve(lib, oracle, opts):
    """first 700 poses of the M3500 demo (360 with inc_fast=0, a full re-plan per step), every step checked"""
    n = 360 if opts.get("inc_fast", 1) == 0 else 700
    r = _run(lib, oracle, opts, lambda L: harness.run_demo(L, datasets.m3500_arrays(), max_poses=n), f"demo {n}")
    assert r["fallback_nodes"] == [k for k in FALLBACKS_700 if k <= n]
    frozen = opts.get("inc_fast", 1) == 1
    if frozen:                                             # the forms the option set targets did run
        assert r["regen2"] > 100, r
    if opts.get("inc_update", 1) and opts.get("inc_multi", 1) and frozen:      # (low-rank updates ride on the multi-level launch)
        assert r["updated"] > 0, r
    else:
        assert r["updated"] == 0, r


def test_full_demo_at_defaults(lib, oracle):
    """the whole 3 500-pose demo, every step checked (stride 1: about 30 s of host time)"""
    import numpy as np
    from tests.conftest import golden
    r = _run(lib, oracle, {}, lambda L: harness.run_demo(L, datasets.m3500_arrays()), "demo 3500")
    assert r["fallback_nodes"] == (np.nonzero(golden("m3500_inc_demo.npz")["was_batch"])[0] + 1).tolist()[1:]    # the reference's 49
    assert r["updated"] > 1000, r


GROWTH = {
    "random_growth_1": lambda L: T._random_growth(L, 1, 140, 25),
    "random_growth_2": lambda L: T._random_growth(L, 2, 140, 10 ** 6),
    "random_growth_3": lambda L: T._random_growth(L, 3, 140, 8),
    "random_growth_old_old": lambda L: T._random_growth(L, 4, 150, 10 ** 6, old_old=True),
    "random_growth_old_old_30": lambda L: T._random_growth(L, 5, 150, 30, old_old=True),
    "recent_growth_28": lambda L: T._recent_pose_growth(L, 11, 120, 10 ** 6, 28),
    "recent_growth_12": lambda L: T._recent_pose_growth(L, 12, 120, 40, 12),
    "recent_growth_9": lambda L: T._recent_pose_growth(L, 13, 120, 10 ** 6, 9),
    "recent_growth_16": lambda L: T._recent_pose_growth(L, 14, 120, 25, 16),
    "late_priors": lambda L: T._growth_with_late_priors(L),
    "tutorial": lambda L: harness.run_tutorial(L),
    "batch_every_37": lambda L: harness.run_demo(L, datasets.m3500_arrays(), max_poses=420, batch_every=37),
}


@pytest.mark.parametrize("opts", [{}, {"inc_update": 0}, {"inc_one": 0}], ids=_ids)
@pytest.mark.parametrize("name", list(GROWTH))
def test_growth_every_step_is_the_exact_solve(lib, oracle, name, opts):
    r = _run(lib, oracle, opts, GROWTH[name], name)
    if "old_old" in name:
        assert r["old_old"] > 0, r
    if name == "random_growth_old_old_30":
        assert r["old_old_cross"] > 0, r
    if name == "batch_every_37":
        assert r["batch"] >= 11, r


@pytest.mark.parametrize("extend", [1, 0])
def test_batch_update_only_every_call_solves_its_normal_equations(lib, oracle, extend):
    """the demo's --batch_update_only mode: one batch call per pose on a growing graph (extended plan or a new plan per call)"""
    chk = IncExact(lib, oracle, log=print)
    with lib.options(batch_extend=extend):
        harness.run_demo(chk, datasets.m3500_arrays(), batch_update_only=True, max_poses=420)
    print(f"[inc-exact] batch_update_only batch_extend={extend}: {chk.summary()}")
    assert chk.report["failures"] == 0 and chk.report["batch"] == 420
