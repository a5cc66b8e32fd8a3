"""Level 0 inside the back substitution's multi-level launch (option persist_leaves, solver_context.inc.h: upload_plan): where only
persist_max_fronts kept the leaves out, they run as the last workgroups of that launch and take x from their parents inside it.  The same
kernel runs on the same data, only a launch boundary goes: states, deltas and l_points must keep the bits of the level-by-level launches
(persist = 0) under k_backsolve_w, for every form of the hand-over (tagged_x), and with everything that is handed over poisoned first.  Under
wave_backsolve = 0 the multi-level launch runs another kernel than the per-level ones: there the states agree to STATE_TOL and chi^2 to
CHI2_TOL of tests/test_gpu_downsweep_handover.py.  The small graphs run as ONE launch per sweep at the default persist_max_fronts; it is
lowered to one front less than they have, so that the count stops the walk above level 0 as it does on M3500."""
import numpy as np
import pytest

from aprilsam_amd import datasets
from tests.support import sweeps
from tests.test_gpu_downsweep_handover import CHI2_TOL, STATE_TOL
import tests.test_gpu_parity as T

pytestmark = pytest.mark.gpu
FORMS = [0, 1, 2]
GRAPHS = ["chain_300", "band_1100", "two_chains_900", "m3500"]
M3500_UPPER_FRONTS = 201                                    # fronts of M3500's levels 1-8: the launch before this option


def _graphs():
    return {"chain_300": T._chain(300, 3), "band_1100": sweeps.structured("band", 1100, 307), "two_chains_900": sweeps.structured("two", 900, 306),
            "m3500": datasets.m3500_batch()}


def resident3(lib, arr, **opts):
    """three resident Gauss-Newton steps on a fresh graph + param: (states, deltas, l_points, chi^2 after, stats)"""
    d = lib.dll
    with lib.options(**opts):
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
        assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 3, 0) == 0
        assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
        chi = d.aprilsam_amd_resident_chi2(g.ptr)
        assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
        out = (g.states(), g.deltas(), g.l_points(), chi, p.stats())
        p.destroy(); g.destroy()
    return out


def _same(a, b, what):
    for k in range(3):
        assert a[k].tobytes() == b[k].tobytes(), (what, ("states", "deltas", "l_points")[k], float(np.max(np.abs(a[k] - b[k]))))


@pytest.fixture(scope="module")
def graphs():
    return _graphs()


@pytest.fixture(scope="module")
def level_by_level(lib, graphs):
    return {k: resident3(lib, arr, persist=0) for k, arr in graphs.items()}


def _cap(name, ref):
    """persist_max_fronts under which the count, and nothing else, stops the walk over the levels above level 0"""
    return {} if name == "m3500" else dict(persist_max_fronts=ref[4]["n_fronts"] - 1)


@pytest.mark.parametrize("name", GRAPHS)
def test_bitwise_against_the_level_by_level_launches(lib, graphs, level_by_level, name):
    ref = level_by_level[name]
    nF = ref[4]["n_fronts"]
    assert ref[4]["dn_launch_fronts"] == 0 and np.isfinite(ref[0]).all()
    for f in FORMS:
        r = resident3(lib, graphs[name], persist_leaves=1, tagged_x=f, wave_backsolve=1, **_cap(name, ref))
        assert r[4]["error_code"] == 0 and r[4]["not_spd"] == 0, (name, f, r[4])
        assert r[4]["dn_launch_fronts"] == nF, (name, f, r[4]["dn_launch_fronts"], nF)            # every front of the tree in the one launch
        _same(r, ref, (name, "tagged_x", f, "against persist 0"))


@pytest.mark.parametrize("name", GRAPHS)
def test_the_other_kernel_within_tolerance(lib, graphs, level_by_level, name):
    ref = level_by_level[name]
    for f in FORMS:
        r = resident3(lib, graphs[name], persist_leaves=1, tagged_x=f, wave_backsolve=0, **_cap(name, ref))
        assert r[4]["error_code"] == 0 and r[4]["not_spd"] == 0 and r[4]["dn_launch_fronts"] == ref[4]["n_fronts"], (name, f, r[4])
        ds, dc = float(np.max(np.abs(r[0] - ref[0]))), abs(r[3] - ref[3]) / max(abs(ref[3]), 1e-12)
        print(f"[persist_leaves] {name} wave_backsolve=0 tagged_x={f}: against persist=0: states {ds:.3e} chi2 {dc:.3e}")
        assert ds < STATE_TOL and dc < CHI2_TOL, (name, f, ds, dc)


@pytest.mark.parametrize("name", GRAPHS)
def test_poisoned_hand_over(lib, graphs, level_by_level, name):
    """pool_poison: NaN into x and every update block before each step.  A leaf that took x before its parent had written it would carry NaN, or
    (granules) the step before's numbers: either way other bits than the clean run's"""
    ref = level_by_level[name]
    for f in FORMS:
        clean = resident3(lib, graphs[name], persist_leaves=1, tagged_x=f, **_cap(name, ref))
        r = resident3(lib, graphs[name], persist_leaves=1, tagged_x=f, pool_poison=1, **_cap(name, ref))
        assert r[4]["error_code"] == 0 and r[4]["dn_launch_fronts"] == ref[4]["n_fronts"] and np.isfinite(r[0]).all() and np.isfinite(r[1]).all()
        _same(r, clean, (name, f, "poisoned against clean"))


def test_not_positive_definite_is_reported_from_the_joined_launch(lib, graphs):
    """the pivot flag's pinned mirror rides on the step's last launch: with the leaves inside, that is the multi-level back substitution"""
    st, fa, fb, z, W = (np.array(a) for a in graphs["chain_300"])
    for k in np.nonzero((fa == 150) | (fb == 150))[0]:         # every factor at pose 150 with negative information: a negative diagonal entry
        W[k] = np.diag([-50.0, 10, 10]).reshape(9)
    nF = T.run_batch(lib, graphs["chain_300"], 1)[2]["n_fronts"]
    with lib.options(persist_leaves=1, persist_max_fronts=nF - 1):
        g = lib.new_graph(); g.build_from_arrays(st, fa, fb, z, W); p = lib.new_param()
        g.cholesky(p)
        s = p.stats()
        assert s["dn_launch_fronts"] == s["n_fronts"] == nF, s
        assert s["not_spd"] == 1, s
        p.destroy(); g.destroy()


def test_option_off_reproduces_the_launches_before(lib, graphs, level_by_level):
    for name in GRAPHS:
        ref = level_by_level[name]
        r = resident3(lib, graphs[name], persist_leaves=0, **_cap(name, ref))
        assert r[4]["error_code"] == 0
        if name == "m3500":
            assert r[4]["dn_launch_fronts"] == M3500_UPPER_FRONTS, r[4]["dn_launch_fronts"]
        else:
            assert 2 <= r[4]["dn_launch_fronts"] < ref[4]["n_fronts"], (name, r[4]["dn_launch_fronts"])      # the cap bites above level 0
        _same(r, ref, (name, "persist_leaves 0 against persist 0"))
