"""Level 0 inside the factorisation's multi-level launch (option persist_up, solver_context.inc.h: upload_plan): where only
persist_max_fronts kept the leaves out and no front changes between its full-LDS and its panel form, the whole tree is factorised by ONE
launch, in level order (1), in descending order of the remaining path (2) or in the order of the slot-aware list schedule (3).  The same
kernel runs on the same data in the same form: states, deltas and l_points must keep the bits of the level-by-level launches (persist = 0),
also with everything that is handed over poisoned first -- a parent that missed a wait then reads NaN.  The small graphs run as ONE launch
per sweep at the default persist_max_fronts; it is lowered to one front less than they have, so that the count stops the walk above level 0
as it does on M3500."""
import numpy as np
import pytest

import tests.test_gpu_parity as T
from tests.test_gpu_persist_leaves import GRAPHS, M3500_UPPER_FRONTS, _cap, _graphs, _same, resident3

pytestmark = pytest.mark.gpu
ORDERS = [1, 2, 3]
# M3500's level 0 as a throughput level whose fronts above 8 KB run in panel mode, at the launch's workgroup size: under the joined
# launch's limit those leaves would run fully in LDS, so the plan must not join
FORM_CHANGE = dict(tp_fronts=300, tp_threads=1024, tp_lds_kb=8)


@pytest.fixture(scope="module")
def graphs():
    return _graphs()


@pytest.fixture(scope="module")
def level_by_level(lib, graphs):
    return {k: resident3(lib, arr, persist=0) for k, arr in graphs.items()}


@pytest.mark.parametrize("name", GRAPHS)
def test_bitwise_against_the_level_by_level_launches(lib, graphs, level_by_level, name):
    ref = level_by_level[name]
    nF = ref[4]["n_fronts"]
    assert ref[4]["up_launch_fronts"] == 0 and np.isfinite(ref[0]).all()
    for o in ORDERS:
        r = resident3(lib, graphs[name], persist_up=o, **_cap(name, ref))
        assert r[4]["error_code"] == 0 and r[4]["not_spd"] == 0, (name, o, r[4])
        assert r[4]["up_launch_fronts"] == nF, (name, o, r[4]["up_launch_fronts"], nF)            # every front of the tree in the one launch
        _same(r, ref, (name, "persist_up", o, "against persist 0"))


@pytest.mark.parametrize("name", GRAPHS)
def test_poisoned_hand_over(lib, graphs, level_by_level, name):
    """pool_poison: NaN into every update block before each step.  A parent that added a leaf's block before the leaf had stored it carries NaN
    or is reported as not positive definite"""
    ref = level_by_level[name]
    for o in ORDERS:
        r = resident3(lib, graphs[name], persist_up=o, pool_poison=1, **_cap(name, ref))
        assert r[4]["error_code"] == 0 and r[4]["not_spd"] == 0 and r[4]["up_launch_fronts"] == ref[4]["n_fronts"], (name, o, r[4])
        assert np.isfinite(r[0]).all() and np.isfinite(r[1]).all()
        _same(r, ref, (name, o, "poisoned against persist 0"))


def test_scheduled_order_without_a_join(lib, graphs, level_by_level):
    """a graph that runs one launch per sweep anyway (the default persist_max_fronts holds it whole) gets the scheduled order too; and neither the
    join nor the order depends on the placed lists being in use (xcd_place = 0: level order is then level 0's own list and the upper fronts')"""
    cases = [("chain_300", dict(persist_up=2)), ("chain_300", dict(persist_up=3))]
    cases += [(name, dict(persist_up=o, xcd_place=0, **_cap(name, level_by_level[name]))) for name in ("chain_300", "m3500") for o in (1, 3)]
    for name, opts in cases:
        ref = level_by_level[name]
        r = resident3(lib, graphs[name], **opts)
        assert r[4]["error_code"] == 0 and r[4]["not_spd"] == 0 and r[4]["up_launch_fronts"] == ref[4]["n_fronts"], (name, opts, r[4])
        _same(r, ref, (name, opts, "against persist 0"))


def test_not_positive_definite_is_reported_through_the_joined_launch(lib, graphs):
    st, fa, fb, z, W = (np.array(a) for a in graphs["chain_300"])
    for k in np.nonzero((fa == 150) | (fb == 150))[0]:         # every factor at pose 150 with negative information: a negative diagonal entry
        W[k] = np.diag([-50.0, 10, 10]).reshape(9)
    nF = T.run_batch(lib, graphs["chain_300"], 1)[2]["n_fronts"]
    for o in ORDERS:
        with lib.options(persist_up=o, persist_max_fronts=nF - 1):
            g = lib.new_graph(); g.build_from_arrays(st, fa, fb, z, W); p = lib.new_param()
            g.cholesky(p)
            s = p.stats()
            assert s["up_launch_fronts"] == s["n_fronts"] == nF, (o, s)
            assert s["not_spd"] == 1, (o, s)
            p.destroy(); g.destroy()


def test_option_off_reproduces_the_launches_before(lib, graphs, level_by_level):
    for name in GRAPHS:
        ref = level_by_level[name]
        r = resident3(lib, graphs[name], persist_up=0, **_cap(name, ref))
        assert r[4]["error_code"] == 0
        if name == "m3500":
            assert r[4]["up_launch_fronts"] == M3500_UPPER_FRONTS, r[4]["up_launch_fronts"]
        else:
            assert 2 <= r[4]["up_launch_fronts"] < ref[4]["n_fronts"], (name, r[4]["up_launch_fronts"])      # the cap bites above level 0
        _same(r, ref, (name, "persist_up 0 against persist 0"))


def test_no_join_where_a_leaf_would_change_form(lib, graphs):
    ref = resident3(lib, graphs["m3500"], persist=0, **FORM_CHANGE)
    assert ref[4]["error_code"] == 0 and np.isfinite(ref[0]).all()
    for o in ORDERS:
        r = resident3(lib, graphs["m3500"], persist_up=o, **FORM_CHANGE)
        assert r[4]["error_code"] == 0 and r[4]["not_spd"] == 0, (o, r[4])
        assert r[4]["up_launch_fronts"] == M3500_UPPER_FRONTS, (o, r[4]["up_launch_fronts"])      # level 0 keeps its own launch
        _same(r, ref, ("m3500", o, "form change: against persist 0"))
