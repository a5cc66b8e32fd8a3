"""The hand-over of x inside the multi-level back substitutions (kernels.hip.h: backsolve_finish, gather_x; option tagged_x): 1 = x travels
from a front to its children as epoch-tagged 16-byte granules and no flag, 0 = write-through x, drained, then a flag, 2 = plain x, an L2
write-back, then the flag (the form before).  The three forms move the same numbers: they must agree BITWISE with each other, in the batch
step's launch (k_backsolve_w, and k_backsolve_t<true> under wave_backsolve = 0) and in the incremental steps' launches.

Against persist = 0 -- one launch per level, no hand-over inside a launch -- the comparison is bitwise where the commit before this file
was: PERSIST_BITWISE_ON_PARENT records that per graph, for k_backsolve_w (the per-level launches pick their kernel and the full / panel
form of a front level by level, the multi-level launch once for all its levels: lattice_40 differs in the last bits, and so does every
graph under wave_backsolve = 0, whose multi-level launch runs k_backsolve_t while the per-level ones keep k_backsolve_w).  There the states agree to STATE_TOL = 1e-5 and chi^2 to CHI2_TOL = 1e-7, the tolerances tests/test_gpu_sweeps.py passes to
tests/support/sweeps.py for such graphs against the oracle."""
import numpy as np
import pytest

from aprilsam_amd import datasets, harness
from tests.support import sweeps
from tests.support.consumer_graphs import three_components, two_components
import tests.test_gpu_parity as T

pytestmark = pytest.mark.gpu
FORMS = [0, 1, 2]
STATE_TOL, CHI2_TOL = 1e-5, 1e-7


def _graphs(lib):
    return {
        "chain_300": T._chain(300, 3),                      # every hop has one child
        "star_70": T._star(70, 2),
        "random_700": datasets.random_pose_graph(700, 600, 21),
        "lattice_60": lib.lattice_arrays(60),               # update blocks of more than 256 rows
        "two_components": two_components()[0],              # several roots, fronts without update rows
        "three_components": three_components()[0],
        # Of the six above only the chain runs the batch step's multi-level launch at the default options (the others have a root front
        # too wide for one workgroup, or leaves with another workgroup size: stats.dn_launch_fronts = 0, their levels run one launch each and
        # nothing is handed over inside a launch).  These four do, all their fronts or their top levels:
        "m3500": datasets.m3500_batch(),                    # 201 fronts of levels 1-8
        "lattice_40": lib.lattice_arrays(40),               # the largest lattice tried whose root still fits one workgroup (fronts of up to 195 rows)
        "band_1100": sweeps.structured("band", 1100, 307),
        "two_chains_900": sweeps.structured("two", 900, 306),      # two roots in one launch, fronts without update rows
    }


GRAPHS = ["chain_300", "star_70", "random_700", "lattice_60", "two_components", "three_components", "m3500", "lattice_40", "band_1100", "two_chains_900"]
IN_ONE_LAUNCH = ("chain_300", "m3500", "lattice_40", "band_1100", "two_chains_900")       # graphs whose back substitution hands x over inside a launch
# persist = 0 against persist = 1 on the commit before this file, three resident steps, states and deltas, k_backsolve_w
# (profiles/r08_downsweep_handover.txt, section 7)
PERSIST_BITWISE_ON_PARENT = {name: name != "lattice_40" for name in GRAPHS}       # (lattice_40: states 2.6e-13, deltas 8.3e-14 apart there)


def resident3(lib, arr, **opts):
    """three resident Gauss-Newton steps on a fresh graph + param: (states, deltas, chi^2 after, stats)"""
    d = lib.dll
    with lib.options(**opts):
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
        assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 3, 0) == 0
        assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
        chi = d.aprilsam_amd_resident_chi2(g.ptr)
        assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
        out = (g.states(), g.deltas(), chi, p.stats())
        p.destroy(); g.destroy()
    return out


def _same(a, b, what):
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (what, float(np.max(np.abs(a[0] - b[0]))), float(np.max(np.abs(a[1] - b[1]))))


@pytest.fixture(scope="module")
def graphs(lib):
    return _graphs(lib)


@pytest.fixture(scope="module")
def level_by_level(lib, graphs):
    return {k: resident3(lib, arr, persist=0) for k, arr in graphs.items()}


@pytest.mark.parametrize("wave", [1, 0], ids=["k_backsolve_w", "k_backsolve_t"])
@pytest.mark.parametrize("name", GRAPHS)
def test_every_form_against_the_level_by_level_launches(lib, graphs, level_by_level, name, wave):
    ref = level_by_level[name]
    assert ref[3]["dn_launch_fronts"] == 0 and np.isfinite(ref[0]).all()
    runs = [resident3(lib, graphs[name], tagged_x=f, wave_backsolve=wave) for f in FORMS]
    for f, r in zip(FORMS, runs):
        assert r[3]["error_code"] == 0 and r[3]["not_spd"] == 0, (name, f, r[3])
        if name in IN_ONE_LAUNCH:
            assert r[3]["dn_launch_fronts"] >= 2, (name, f, r[3]["dn_launch_fronts"])        # the multi-level launch ran: x was handed over inside it
            assert 3 * (r[3]["max_front_rows"] // 3 - 1) <= 256                               # ... by lanes that gather one row each
        else:                                                                                 # (the day the planner changes that, these cases start to count)
            assert r[3]["dn_launch_fronts"] == 0, (name, f, r[3]["dn_launch_fronts"])
        _same(r, runs[0], (name, "tagged_x", f, "against tagged_x 0"))
        ds, dc = float(np.max(np.abs(r[0] - ref[0]))), abs(r[2] - ref[2]) / max(abs(ref[2]), 1e-12)
        print(f"[handover] {name} wave_backsolve={wave} tagged_x={f}: {r[3]['dn_launch_fronts']} fronts in the launch, against persist=0: states {ds:.3e} chi2 {dc:.3e}")
        if PERSIST_BITWISE_ON_PARENT[name] and wave == 1:
            _same(r, ref, (name, "tagged_x", f, "against persist 0"))
        else:                                                                  # (k_backsolve_t sums in another order than the per-level launches' kernel)
            assert ds < STATE_TOL and dc < CHI2_TOL, (name, f, ds, dc)


@pytest.mark.parametrize("form", [0, 1])
def test_stale_tags_of_another_plan(lib, graphs, form):
    """two graphs solved alternately on ONE param: every call re-plans and finds the granules, the flags and x of the other graph's steps"""
    a, b = graphs["m3500"], graphs["chain_300"]
    with lib.options(tagged_x=form):
        fresh = []
        for arr in (a, b):
            g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
            g.cholesky(p); g.cholesky(p)
            fresh.append((g.states(), g.deltas())); p.destroy(); g.destroy()
        p = lib.new_param()
        for rnd in range(3):
            for arr, want in zip((a, b), fresh):
                g = lib.new_graph(); g.build_from_arrays(*arr)
                g.cholesky(p); g.cholesky(p)
                s = p.stats()
                assert s["error_code"] == 0 and s["dn_launch_fronts"] >= 2, s
                _same((g.states(), g.deltas()), want, ("round", rnd, len(arr[0])))
                g.destroy()
        p.destroy()


def test_constant_granules_of_a_smaller_plan(lib, graphs):
    """a plan marks the granules behind its last pose as constant zeros (what phantom rows of an incremental step's tail front read).  The next,
    larger plan on the same param owns that position: the mark must be gone, or the children of the front that owns it take 0 for its x"""
    big = graphs["chain_300"]
    with lib.options(tagged_x=1, batch_extend=0):
        g = lib.new_graph(); g.build_from_arrays(*big); p = lib.new_param()
        g.cholesky(p)
        want = (g.states(), g.deltas()); p.destroy(); g.destroy()
        p = lib.new_param()
        for k in range(100, 160, 3):                        # (one pose in eight of a chain is a separator: several of these positions are)
            for arr in (T._chain(k, 3), big):
                g = lib.new_graph(); g.build_from_arrays(*arr)
                g.cholesky(p)
                assert p.stats()["error_code"] == 0 and p.stats()["dn_launch_fronts"] >= 2
                got = (g.states(), g.deltas()); g.destroy()
            _same(got, want, ("after a plan of", k, "poses"))
        p.destroy()


def test_incremental_multi_level_launches(lib):
    """first 700 poses of the M3500 demo, every step through the flag-synchronised launches (inc_one = 0, inc_tail = 0): the three forms
    bitwise after every step"""
    arr = datasets.m3500_arrays()
    runs = []
    for f in FORMS:
        multi = []
        with lib.options(tagged_x=f, inc_one=0, inc_tail=0):
            r = harness.run_demo(lib, arr, max_poses=700, record_states_every=1, on_step=lambda k, p, batch: multi.append(0 if batch else p.stats()["dn_launch_fronts"]))
        print(f"[handover] incremental demo, tagged_x={f}: {sum(1 for n in multi if n >= 2)} steps with a multi-level back substitution")
        assert sum(1 for n in multi if n >= 2) > 0                             # the multi-level down-sweep form ran
        runs.append(r)
    for f, r in zip(FORMS[1:], runs[1:]):
        assert np.array_equal(r["was_batch"], runs[0]["was_batch"]) and r["chi2"].tobytes() == runs[0]["chi2"].tobytes(), f
        for k in range(700):
            assert r["snaps"][k].tobytes() == runs[0]["snaps"][k].tobytes(), (f, k)


@pytest.mark.parametrize("form", FORMS)
def test_poisoned_hand_over_is_finite_and_correct(lib, graphs, level_by_level, form):
    """pool_poison fills x and every update block with NaN before each step (skip_flag_waits stays off: every wait is in place).  A flag wait
    that passed early would hand a child NaN; the granules are not poisoned, so a poll that passed early would hand it the x of the step
    before -- either way the result differs from the clean run's, which is what is compared, bit for bit"""
    for name in ("chain_300", "m3500"):
        r = resident3(lib, graphs[name], tagged_x=form, pool_poison=1, skip_flag_waits=0)
        assert r[3]["error_code"] == 0 and np.isfinite(r[0]).all() and np.isfinite(r[1]).all()
        _same(r, resident3(lib, graphs[name], tagged_x=form), (name, form, "poisoned against clean"))


def _closure_growth(lib, n_old, n_new, seed):
    """one pose, then n_old + n_new poses added one incremental step each (no re-plan: every front is a tail front of at most 8 poses, option
    tail_poses); each of the last n_new poses also closes a loop to one of the first n_old.  The tail fronts that own those old poses collect
    one update row block per closing pose: fronts of few columns and far more than 256 update rows, inside the steps' multi-level launches.
    Returns the states after every step and (fronts in the step's multi-level back substitution, rows of the tallest front so far) per step"""
    rng = np.random.default_rng(seed)
    g = lib.new_graph(); p = lib.new_param(nthreshold=10 ** 6, delta_xy=0.05, delta_theta=0.05)
    W = np.diag([40.0, 40.0, 120.0])
    truth = [np.zeros(3)]
    g.add_node_xyt(truth[0]); g.add_factor_xytpos(0, [0, 0, 0], datasets.PRIOR_W)
    g.cholesky(p)

    def rel(a, b):
        c, s_ = np.cos(a[2]), np.sin(a[2]); dx, dy = b[0] - a[0], b[1] - a[1]
        return np.array([c * dx + s_ * dy, -s_ * dx + c * dy, b[2] - a[2]])
    states, seen = [], []
    for n in range(1, n_old + n_new + 1):
        last = truth[-1]
        new = np.array([last[0] + np.cos(last[2]) * 0.8, last[1] + np.sin(last[2]) * 0.8, last[2] + rng.uniform(-0.5, 0.5)])
        truth.append(new)
        g.add_node_xyt(new + rng.normal(0, [0.1, 0.1, 0.03]))
        g.add_factor_xyt(n - 1, n, rel(truth[n - 1], new) + rng.normal(0, [0.03, 0.03, 0.01]), W)
        if n > n_old:
            o = int(rng.integers(0, n_old))
            g.add_factor_xyt(o, n, rel(truth[o], new) + rng.normal(0, [0.03, 0.03, 0.01]), W)
        p.c.batch_time = 1e300
        g.cholesky_inc(p)
        st = p.stats()
        assert st["error_code"] == 0, (n, st)
        seen.append((st["dn_launch_fronts"], st["max_front_rows"]))
        states.append(g.states())
    p.destroy(); g.destroy()
    return states, seen


def test_update_blocks_of_more_than_256_rows(lib):
    """a lane gathers ONE granule: a launch that holds a front of more than 256 update rows has to take the flag form (launch_xmode), or the
    rows past the 256th never reach the front.  No batch plan found puts such a front into a multi-level launch (profiles/r08_downsweep_handover.txt,
    section 9); incremental steps do once the low-rank updates are off (inc_update = 0: with them a front that tall makes the step re-plan at
    about 85 update blocks) -- here the fronts of at most 8 poses (24 columns) that own the first 24 poses collect 120 closing poses, so the
    last 26 or so steps (from the 94th closing pose on: 3 * 94 - 24 > 256) hold a front of more than 256 update rows"""
    runs = {}
    for f in FORMS:
        with lib.options(tagged_x=f, tail_poses=8, inc_one=0, inc_tail=0, inc_update=0):
            runs[f] = _closure_growth(lib, 24, 120, 5)
    seen = runs[1][1]
    tall = [k for k, (n, rows) in enumerate(seen) if n >= 2 and rows - 3 * 8 > 256]      # (a front owns at most 8 poses: the rest of its rows are update rows)
    print(f"[handover] closure growth: tallest front {max(r for _, r in seen)} rows; {len(tall)} steps ran a multi-level back substitution holding a front of more than 256 update rows")
    assert len(tall) >= 10, (len(tall), seen[-1])
    for f in (0, 1):
        assert runs[f][1] == runs[2][1], f
        for k, (a, b) in enumerate(zip(runs[f][0], runs[2][0])):
            assert np.isfinite(a).all() and a.tobytes() == b.tobytes(), (f, k, float(np.max(np.abs(a - b))))
