"""The placement model of tests/support/pivot_placement.py (no GPU): every position class exists under every plan the GPU tests use,
the knob puts the first non-positive pivot where it says, and float64 agrees with a longer LDL' (numpy.longdouble) on what it places."""
import numpy as np
import pytest
import scipy.linalg as sla

from tests.support import pivot_placement as pp

LONG = np.finfo(np.longdouble).eps < 1e-18       # (x87 extended or better; on a platform where longdouble is double the comparison is void)


@pytest.fixture(scope="module")
def lam(lib):
    p = lib.new_param(); v = float(p.c.tikhanov); p.destroy()
    return v


@pytest.mark.parametrize("leaf_nodes", pp.PLANS)
def test_every_position_class_is_present_under_every_plan(lib, lam, leaf_nodes):
    tab, missing = pp.class_table(lib, leaf_nodes, lam)
    assert missing == [], (leaf_nodes, missing)
    for k, (pl, t, c) in tab.items():
        ns, lev = int(pl.ns[t]), int(pl.level[t])
        assert 0 <= c < ns
        if k == "leaf_c0":
            assert lev == 0 and c == 0
        elif k == "blk_first":
            assert c % 16 == 0 and c > 0
        elif k == "blk_last":
            assert c % 16 == 15
        elif k == "interior":
            assert 1 <= c % 16 <= 14 and c < ns - 1
        elif k == "partial_last":
            assert c == ns - 1 and ns % 16 != 0
        elif k == "middle_level":
            assert 0 < lev < int(pl.level.max())
        elif k == "root_last":
            assert int(pl.first[t]) + c == pl.n - 1
        else:
            assert ns > 128
            ob, panel, m = c // 128, (c % 128) // 32, c % 32
            want = dict(big_ob0_p0_m0=(0, 0, 0), big_ob0_p3_m31=(0, 3, 31), big_ob1_p0_mid=(1, 0, 7), big_ob1_p3_m0=(1, 3, 0))
            if k in want:
                assert (ob, panel, m) == want[k]
            else:
                assert c == ns - 1 and ns % 32 != 0
    # the graphs with several roots and with a tiny root offer the decisive position too
    for name in pp.GRAPHS:
        assert "root_last" in pp.placement(lib, name, leaf_nodes, lam).classes()


@pytest.mark.parametrize("leaf_nodes", pp.PLANS)
def test_the_knob_places_the_first_non_positive_pivot(lib, lam, leaf_nodes):
    """A0 - s e_p e_p' in the plan's order: the pivots before p are A0's (same leading block), pivot p = -delta d_p, and the diagonal entry
    A_pp - s stays positive wherever elimination has taken more than delta / (1 + delta) of A_pp -- at the last pivot of every graph's last
    front in particular ("indefinite with a positive diagonal")"""
    tab, _ = pp.class_table(lib, leaf_nodes, lam)
    for k, (pl, t, c) in tab.items():
        cs = pl.case(t, c)
        p = cs["p"]
        A1 = pl.matrix(p, cs["s"])
        assert np.array_equal(A1[:p, :p], pl.A0[:p, :p]) and np.all(pl.d[:p] > 0)      # the leading block, so every earlier pivot, is A0's
        v = sla.solve_triangular(np.linalg.cholesky(pl.A0[:p, :p]), pl.A0[:p, p], lower=True) if p else np.zeros(0)
        piv0, piv1 = pl.A0[p, p] - v @ v, A1[p, p] - v @ v
        assert piv0 == pytest.approx(cs["d_p"], rel=1e-9)
        assert piv1 == pytest.approx(-pp.DELTA * cs["d_p"], rel=1e-8), (k, piv1, cs["d_p"])
        if k in ("root_last", "partial_last", "big_partial_last", "big_ob1_p3_m0"):     # the fill has taken more than delta / (1 + delta) of the entry
            assert cs["diag"] > 0, (k, cs["diag"])
        assert (cs["diag"] > 0) == (pl.A0[p, p] > (1 + pp.DELTA) * cs["d_p"])
        # the knob is the last factor of the returned arrays, residual exactly 0
        st, fa, fb, z, W = cs["arr"]
        assert fa[-1] == cs["node"] and fb[-1] == -1 and np.array_equal(z[-1], st[cs["node"]]) and W[-1][4 * cs["comp"]] == -cs["s"]
        assert pl.s_star(p) <= cs["d_p"] * (1 + 1e-9)
    for name in pp.GRAPHS:                        # the decisive position of every graph: a positive diagonal entry over a negative pivot
        pl = pp.placement(lib, name, leaf_nodes, lam)
        assert pl.case(*pl.classes()["root_last"])["diag"] > 0


def test_float64_placement_against_the_longer_reference(lib, lam):
    """The chain (270 scalars) under the three plans: float64 LDL' against LDL' in numpy.longdouble (64-bit mantissa) on the same matrix.

    delta = 0.25: same index of the first non-positive pivot, for every class the chain offers and for every 19th scalar position.
    delta = 1e-6: same sign of the smallest pivot (knob at (1 +- delta) s*).
    Measured (x86-64, 80-bit longdouble): worst relative difference of d_p between the two over all positions and plans 1.5e-11 (the chain
    hangs on one prior at its far end: cond(A0) = 5.7e7; the bound asserted is n eps cond(A0) = 3.4e-6)."""
    assert LONG, "numpy.longdouble is no longer than float64 on this platform: the longer reference needs a 64-bit mantissa"
    worst = 0.0
    for leaf_nodes in pp.PLANS:
        pl = pp.placement(lib, "chain", leaf_nodes, lam)
        assert pl.n <= 300
        dl = pp.ldl_pivots(pl.A0, np.longdouble)
        worst = max(worst, float(np.max(np.abs(pl.d.astype(np.longdouble) - dl) / dl)))
        positions = sorted(set(int(pl.first[t]) + c for t, c in pl.classes().values()) | set(range(0, pl.n, 19)) | {pl.n - 1})
        for p in positions:
            A = pl.matrix(p, (1 + pp.DELTA) * pl.d[p])
            i64 = pp.first_non_positive(pp.ldl_pivots(A, np.float64, stop_at_first=True))
            il = pp.first_non_positive(pp.ldl_pivots(A, np.longdouble, stop_at_first=True))
            assert i64 == il == p, (leaf_nodes, p, i64, il)
        for p in positions[::7] + [pl.n - 1]:
            ss = pl.s_star(p)
            for sign in (+1, -1):
                A = pl.matrix(p, (1 + sign * 1e-6) * ss)
                m64 = np.nanmin(pp.ldl_pivots(A, np.float64)); ml = np.nanmin(pp.ldl_pivots(A, np.longdouble))
                assert (m64 > 0) == (ml > 0) == (sign < 0), (leaf_nodes, p, sign, m64, ml)
    print(f"worst relative |d_p(float64) - d_p(longdouble)| = {worst:.2e}")
    assert worst < pl.n * np.finfo(float).eps * np.linalg.cond(pl.A0), worst


def test_refined_reference_converges(lib, lam):
    """the yardstick of the no-false-alarm case: the refined solve's residual, evaluated in longdouble, is at longdouble rounding level"""
    assert LONG, "numpy.longdouble is no longer than float64 on this platform: the longer reference needs a 64-bit mantissa"
    pl = pp.placement(lib, "chain", 16, lam)
    p = pl.n - 1
    A = pl.matrix(p, (1 - 1e-6) * pl.s_star(p))
    x, x0 = pp.refined_solve(A, pl.b)
    Al = A.astype(np.longdouble)
    r = pl.b.astype(np.longdouble) - Al @ x
    scale = np.abs(Al) @ np.abs(x) + np.abs(pl.b)
    assert float(np.max(np.abs(r) / scale)) < 1e-17
    assert float(np.max(np.abs(x0 - x))) <= pl.n * np.finfo(float).eps * np.linalg.cond(A) * float(np.max(np.abs(x)))      # (the plain solve: n eps cond)
