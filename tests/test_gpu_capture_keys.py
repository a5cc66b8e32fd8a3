"""What a captured hipGraph depends on (DESIGN.md sections 12, 15, 19, 20 and 17): one param driven through a fixed sequence of resident
steps, API calls, LM iterations, an edit in place, an appended factor, a node fixed and freed again and a GNC run, on a 40-pose loop with
a robust, a max-mixture (K = 2) and a polar closure.  After every step the number of graphs captured so far is the recorded one, the same
sequence without graphs captures none, and both leave the same states bit for bit (a replay changes no arithmetic: the kernels and
their order are the same -- the neighbouring use_graph=0 tests of LM, chordal and the robust steps assert the same).

A characterisation test: EXPECTED was recorded on commit 362a7eb ("Add aprilsam_amd_factor_audit: per-factor leverage and
leave-one-out"), before the capture keys were gathered into one mechanism, and is not to be re-recorded from later code."""
import numpy as np
import pytest

from aprilsam_amd import abi
from tests.support import maxmix_model as mm
from tests.support import polar_model as pm
from tests.support import robust_model as rm

pytestmark = pytest.mark.gpu
N = 40
LANDMARK = N                       # node 40: seen from pose 12 (range and bearing); tikhanov keeps its heading regular
PLAIN_CLOSURES = [(0, 39), (3, 30), (10, 25)]
ROBUST_CLOSURE, MAX_CLOSURE, LATE_ROBUST = (5, 35), (8, 28), (15, 33)

# graphs captured so far, after each step of _sequence(), recorded on 362a7eb (see the module's docstring)
EXPECTED = [("resident step 1", 1), ("resident step 2", 1), ("resident step 3", 1),
            ("API call 1", 1), ("API call 2", 2), ("API call 3", 2),
            ("LM, two iterations", 3),
            ("API call 4, robust scale edited", 3), ("API call 5", 3), ("API call 6", 3),
            ("resident step, robust factor appended", 4),
            ("resident step, node 7 fixed", 5),
            ("resident step, node 7 free", 6),
            ("GNC, two stages", 7),
            ("LM, two iterations more", 8)]


def _scene():
    rng = np.random.default_rng(5)
    a = 2.0 * np.pi * np.arange(N) / N
    truth = np.column_stack([5.0 * np.cos(a), 5.0 * np.sin(a), pm.mod2pi(a + 0.5 * np.pi)])
    truth = np.vstack([truth, [0.5, -0.25, 0.0]])
    start = truth + np.column_stack([rng.normal(0, 0.05, (N + 1, 2)), rng.normal(0, 0.02, N + 1)])
    W = np.diag([100.0, 100.0, 400.0])

    def meas(i, j):
        q, _, _ = pm.rel(truth[i], truth[j])
        return np.array([q[0] + rng.normal(0, 0.02), q[1] + rng.normal(0, 0.02), pm.mod2pi(truth[j, 2] - truth[i, 2] + rng.normal(0, 0.01))])
    pairs = [(i, i + 1) for i in range(N - 1)] + PLAIN_CLOSURES + [ROBUST_CLOSURE, MAX_CLOSURE, LATE_ROBUST]
    z = {p: meas(*p) for p in pairs}
    zp = pm.h(pm.RANGE_BEARING, pm.rel(truth[12], truth[LANDMARK])[0]) + rng.normal(0, 0.01, 2)
    return dict(start=start, W=W, z=z, zp=zp, Wp=np.diag([2500.0, 10000.0]))


def _build(lib, sc):
    """-> graph, the index of the robust closure, the indices of the plain closures (GNC's candidates)"""
    g = lib.new_graph()
    for s in sc["start"]:
        g.add_node_xyt(s)
    g.add_factor_xytpos(0, sc["start"][0], sc["W"])
    for i in range(N - 1):
        g.add_factor_xyt(i, i + 1, sc["z"][(i, i + 1)], sc["W"])
    cand = []
    for p in PLAIN_CLOSURES:
        g.add_factor_xyt(*p, sc["z"][p], sc["W"]); cand.append(g.n_factors - 1)
    g.add_factor_xyt(*ROBUST_CLOSURE, sc["z"][ROBUST_CLOSURE], sc["W"])
    rb = g.n_factors - 1
    assert g.set_robust(rb, rm.CAUCHY, 1.0) == 0
    g.add_factor_max(*MAX_CLOSURE, *mm.two_component(sc["z"][MAX_CLOSURE], sc["W"]))
    g.add_factor_polar(abi.POLAR_RANGE_BEARING, 12, LANDMARK, sc["zp"], sc["Wp"])
    return g, rb, cand


def _sequence(lib, sc):
    """-> [(step, graphs captured so far, states after it)]"""
    d = lib.dll
    g, rb, cand = _build(lib, sc)
    p = lib.new_param()
    log = []

    def note(what):
        log.append((what, p.graph_captures(), g.states().copy()))

    def resident(n, what):
        assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
        for k in range(n):
            assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 1, 0) == 0
            if k < n - 1:
                log.append((f"{what} {k + 1}", p.graph_captures(), None))      # (the states are on the device until the loop ends)
        assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
        assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
        note(f"{what} {n}" if n > 1 else what)

    resident(3, "resident step")
    for k in range(3):
        g.cholesky(p); note(f"API call {k + 1}")
    g.optimize_lm(p, max_iters=2); note("LM, two iterations")
    assert g.set_robust(rb, rm.CAUCHY, 2.0) == 0                               # an edit in place: the table is uploaded again where it lies
    g.cholesky(p); note("API call 4, robust scale edited")
    for k in (5, 6):
        g.cholesky(p); note(f"API call {k}")
    g.add_factor_xyt(*LATE_ROBUST, sc["z"][LATE_ROBUST], sc["W"])
    assert g.set_robust(g.n_factors - 1, rm.HUBER, 1.5) == 0
    resident(1, "resident step, robust factor appended")
    assert g.set_fixed(7, True) == 0
    resident(1, "resident step, node 7 fixed")
    assert g.set_fixed(7, False) == 0
    resident(1, "resident step, node 7 free")
    r = g.optimize_gnc(p, cand, c=0.1, max_stages=2, max_iters=3)      # (c far below the residuals: mu starts high, two stages do not end it)
    assert r["stages"] == 2
    note("GNC, two stages")
    g.optimize_lm(p, max_iters=2); note("LM, two iterations more")
    p.destroy(); g.destroy()
    return log


def test_capture_counts_and_states_of_a_fixed_sequence(lib):
    sc = _scene()
    with_graphs = _sequence(lib, sc)
    with lib.options(use_graph=0):
        without = _sequence(lib, sc)
    print("captures:", [(w, n) for w, n, _ in with_graphs])
    assert [w for w, _, _ in without] == [w for w, _, _ in with_graphs]
    assert all(n == 0 for _, n, _ in without), [(w, n) for w, n, _ in without]
    for (what, _, a), (_, _, b) in zip(with_graphs, without):
        if a is not None:
            assert np.all(np.isfinite(a)) and a.tobytes() == b.tobytes(), (what, np.abs(a - b).max())
    assert [(w, n) for w, n, _ in with_graphs] == EXPECTED
