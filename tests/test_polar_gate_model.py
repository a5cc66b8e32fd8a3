"""The numpy model of the polar gates (tests/support/polar_gate_model.py) checked against central differences and
against the already-pinned xyt gate (tests/support/gate_model.py), and the association case the GPU test reuses: its seeds are picked here,
on the CPU, so that index equality on the GPU cannot hinge on round-off.  No GPU, no library."""
import numpy as np
import pytest

from tests.support import gate_model
from tests.support import polar_gate_model as pg
from tests.support import polar_model as pm

KINDS = (pm.RANGE, pm.BEARING, pm.RANGE_BEARING)


def _spd(rng, n, scale=1.0):
    M = rng.normal(size=(n, n))
    return scale * (M @ M.T + n * np.eye(n))


@pytest.mark.parametrize("kind", KINDS)
def test_jacobian_equals_central_differences(kind):
    rng = np.random.default_rng(kind)
    worst = 0.0
    for _ in range(50):
        pa = rng.normal(0, [3, 3, 2]); pb = pa + np.r_[rng.uniform(0.3, 4.0) * np.array([np.cos(t := rng.uniform(-np.pi, np.pi)), np.sin(t)]), rng.normal()]
        J = pg.jacobian(kind, pa, pb)
        x = np.r_[pa, pb]
        num = np.zeros_like(J)
        for k in range(6):
            e = np.zeros(6); e[k] = 1e-6
            hp = pm.h(kind, gate_model.predict((x + e)[:3], (x + e)[3:])[:2]); hm = pm.h(kind, gate_model.predict((x - e)[:3], (x - e)[3:])[:2])
            d = hp - hm
            if kind != pm.RANGE:
                d[-1] = (d[-1] + np.pi) % (2 * np.pi) - np.pi
            num[:, k] = d / 2e-6
        worst = max(worst, np.abs(J - num).max() / max(1.0, np.abs(J).max()))
        assert np.all(J[:, 5] == 0)                               # b's heading is not observed
    print(f"kind {kind}: J_p against central differences, worst {worst:.3e}")
    assert worst < 1e-7                                             # (h = 1e-6: truncation h^2 |h'''| and round-off eps / h, both ~1e-10 times |J| <= 10)


def test_range_bearing_gate_is_the_xyt_gate_in_polar_coordinates():
    """G S_xyt[:2, :2] G' with W_xyt^-1[:2, :2] mapped the same way is the model's S, and -- for the twin whose first two residuals are
    G^-1 r_p -- the d2 of those two rows is the model's d2"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(100):
        pa = rng.normal(0, [3, 3, 2]); t = rng.uniform(-np.pi, np.pi)
        pb = pa + np.r_[rng.uniform(0.3, 4.0) * np.array([np.cos(t), np.sin(t)]), rng.normal()]
        C = _spd(rng, 6, 1e-3)
        W3 = _spd(rng, 3, 50.0)
        q = gate_model.predict(pa, pb)
        G = pm.G(pm.RANGE_BEARING, q[:2])
        Wp = np.linalg.inv(G @ np.linalg.inv(W3)[:2, :2] @ G.T)
        z = pm.h(pm.RANGE_BEARING, q[:2]) + rng.normal(0, [0.05, 0.03])
        ok, d2, S = pg.gate_one(pm.RANGE_BEARING, z, Wp, pa, pb, C)
        rp = pm.residual(pm.RANGE_BEARING, z, q[:2])
        z3 = np.r_[q[:2] + np.linalg.solve(G, rp), q[2]]           # the twin: its first two residuals are G^-1 r_p, its heading residual zero
        d2x, Sx = gate_model.gate(np.array([pa, pb]), [0], [1], [z3], [W3.reshape(9)], [C])
        _, _, rx = gate_model.jacobians(pa, pb, z3)
        assert ok and rx[2] == 0.0
        S2 = Sx[0][:2, :2]
        worst = max(worst, np.abs(G @ S2 @ G.T - S).max() / np.abs(S).max(), abs(rx[:2] @ np.linalg.solve(S2, rx[:2]) - d2) / d2)
    print(f"model against the xyt gate in polar coordinates: worst {worst:.3e}")
    assert worst < 1e-10                                            # (two 2 x 2 solves and a 6 x 6 product in double: cond(S) < 1e3 here)


def test_zero_range_is_unavailable():
    for kind in KINDS:
        ok, d2, S = pg.gate_one(kind, [1.0, 0.2], np.eye(pm.rows(kind)), [1.0, 2.0, 0.3], [1.0, 2.0, -1.0], np.eye(6))
        assert not ok and np.isnan(d2) and np.isnan(S).all() and S.shape == (pm.rows(kind),) * 2


@pytest.fixture(scope="module")
def case():
    c = pg.association_case()
    d = c["d"]
    Sig = pg.dense_sigma(c["x"], d["plain"], d["polars"], pm.TIKHANOV)
    J = pg.joint_blocks(Sig, [c["observer"]] * len(c["landmarks"]), c["landmarks"])
    return c, J


def test_pinned_association_case(case):
    c, J = case
    assert c["d"]["n_poses"] == 6 and len(c["landmarks"]) == 8 and len(c["obs"]) >= 6
    assert {o[0] for o in c["obs"]} == set(KINDS)
    r = pg.associate(c["x"], c["observer"], c["obs"], c["landmarks"], J)
    assert np.array_equal(r["best"], c["truth_idx"]), (r["best"], c["truth_idx"])      # every observation's true landmark is the nearest, inside its gate
    gap = (r["d2_second"] - r["d2_best"]) / r["d2_second"]
    print(f"pinned case: d2_best {r['d2_best']}, relative gap to the second {gap}")
    assert np.all(gap > 1e-6) and r["unavailable"] == 0


def test_association_rules(case):
    c, J = case
    x, o, lm = c["x"], c["observer"], c["landmarks"]
    # a landmark listed twice: the lower index
    lm2 = np.r_[lm, lm[:3]]; J2 = np.concatenate([J, J[:3]])
    r = pg.associate(x, o, c["obs"], lm2, J2)
    assert np.array_equal(r["best"], c["truth_idx"])
    twice = c["truth_idx"] < 3
    assert twice.any() and np.array_equal(r["d2_second"][twice], r["d2_best"][twice])
    # L = 1 and L = 0
    r = pg.associate(x, o, c["obs"], lm[:1], J[:1])
    assert np.all(np.isinf(r["d2_second"])) and np.all(np.isfinite(r["d2_best"]))
    r = pg.associate(x, o, c["obs"], lm[:0], J[:0])
    assert np.all(r["best"] == -1) and np.all(np.isinf(r["d2_best"])) and np.all(np.isinf(r["d2_second"]))
    # far from every landmark: no match, a finite d2_best
    far = [(pm.RANGE_BEARING, np.array([40.0, 0.3]), c["obs"][0][2])]
    r = pg.associate(x, o, far, lm, J)
    assert r["best"][0] == -1 and np.isfinite(r["d2_best"][0]) and r["d2_best"][0] > pg.CHI2_2_999
    # a landmark standing on the observer: skipped, counted
    xs = x.copy(); xs[lm[2], :2] = xs[o, :2]
    r = pg.associate(xs, o, c["obs"], lm, J)
    assert r["unavailable"] == len(c["obs"]) and np.isnan(r["d2"][:, 2]).all() and np.all(r["best"] != 2)


def test_quantiles():
    assert abs(pg.CHI2_1_999 - 10.827566170662733) < 1e-9 and abs(pg.CHI2_2_999 - 13.815510557964274) < 1e-9
