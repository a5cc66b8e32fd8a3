"""Robust losses on xyt / xytpos factors, host side: the formulas of the numpy model, set / get / clear and every
refusal of aprilsam_amd_factor_set_robust, deep copies, the library's host eval / state_eval against the model, .graph saving, the
model's IRLS against the unmodified reference driving the independent checker factor (tests/support/robust_factor.c), and the model's
LM decrease.  No GPU."""
import ctypes as C
import os
from decimal import Decimal, localcontext

import numpy as np
import pytest

from aprilsam_amd import abi
from tests.support import lm_model
from tests.support import maxmix_model as mm
from tests.support import robust_model as rm


class Eval(C.Structure):
    _fields_ = [("chi2", C.c_double), ("jacobians", C.POINTER(C.POINTER(abi.Matd3x3))), ("length", C.c_int),
                ("r", C.POINTER(C.c_double)), ("W", C.POINTER(abi.Matd3x3))]


_EVAL = C.CFUNCTYPE(C.POINTER(Eval), C.c_void_p, C.c_void_p, C.c_void_p)
_COPY = C.CFUNCTYPE(C.POINTER(abi.Factor), C.c_void_p)
KINDS = (rm.HUBER, rm.CAUCHY, rm.DCS)


def _call_eval(f, g, which):
    fn = _EVAL(getattr(f, which))
    return fn(C.cast(C.pointer(f), C.c_void_p), C.cast(g.ptr, C.c_void_p), None)


def _spd(rng):
    M = rng.normal(size=(3, 3))
    W = M @ M.T + np.diag(rng.uniform(1, 20, 3))
    return 0.5 * (W + W.T)


def _small_graph(lib, rng, n=4):
    g = lib.new_graph()
    for i in range(n):
        g.add_node_xyt(rng.normal(0, 2, 3))
    g.add_factor_xytpos(0, [0.1, -0.2, 0.3], _spd(rng))
    for i in range(1, n):
        g.add_factor_xyt(i - 1, i, rng.normal(0, 1, 3), _spd(rng))
    return g


# ---- 1. formulas ---------------------------------------------------------------------------------------------------------------
def _rho_dec(kind, c, s):
    """rho in 50-digit decimal arithmetic (the float model's cancellation would swamp a central difference where w is tiny)"""
    c = Decimal(c); cc = c * c
    if kind == rm.HUBER:
        return s if s <= cc else 2 * c * s.sqrt() - cc
    if kind == rm.CAUCHY:
        return cc * (1 + s / cc).ln()
    return s if s <= cc else cc * (3 * s - cc) / (s + cc)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", [0.3, 1.0, 7.0])
def test_weight_is_the_derivative_of_rho(kind, c):
    s = np.logspace(-8, 8, 161)
    s = s[np.abs(s - c * c) > 1e-6 * c * c]           # (central differences straddling the threshold are one-sided derivatives)
    w = rm.weight(kind, c, s)
    with localcontext() as ctx:
        ctx.prec = 50
        for si, wi, ri in zip(s, w, rm.rho(kind, c, s)):
            S = Decimal(float(si)); h = S * Decimal("1e-15")
            d = (_rho_dec(kind, c, S + h) - _rho_dec(kind, c, S - h)) / (2 * h)
            assert abs(float(d) - wi) <= 1e-8 * wi, (si, float(d), wi)
            assert abs(float(_rho_dec(kind, c, S)) - ri) <= 1e-14 * ri, (si, ri)
    assert np.all(w > 0) and np.all(w <= 1)
    assert np.all(rm.rho(kind, c, s) <= s)
    # continuity of rho and w at the threshold c^2
    t = c * c
    for f in (rm.rho, rm.weight):
        lo, hi = f(kind, c, t * (1 - 1e-12)), f(kind, c, t * (1 + 1e-12))
        assert abs(hi - lo) <= 1e-9 * max(abs(lo), 1e-300)
    # NaN in, NaN out
    assert np.isnan(rm.weight(kind, c, np.nan)) and np.isnan(rm.rho(kind, c, np.nan))


def test_none_is_the_plain_loss():
    s = np.logspace(-3, 3, 13)
    assert np.all(rm.rho(rm.NONE, 1.0, s) == s) and np.all(rm.weight(rm.NONE, 1.0, s) == 1.0)


# ---- 2. the API ----------------------------------------------------------------------------------------------------------------
def test_set_get_clear(lib):
    g = _small_graph(lib, np.random.default_rng(1))
    assert g.get_robust(1) == (rm.NONE, 0.0)
    for i, kind in enumerate(KINDS):
        assert g.set_robust(i, kind, 0.5 + i) == 0
        assert g.get_robust(i) == (kind, 0.5 + i)
    assert g.set_robust(0, rm.CAUCHY, 2.5) == 0 and g.get_robust(0) == (rm.CAUCHY, 2.5)      # (re-set: replaced)
    assert g.set_robust(0, rm.NONE, 0.0) == 0 and g.get_robust(0) == (rm.NONE, 0.0)
    assert lib.dll.aprilsam_amd_factor_get_robust(None, None, None) == 0
    g.destroy()


@pytest.mark.parametrize("case", ["foreign", "max", "max_of_robust", "asym", "indefinite", "kind_low", "kind_high", "c0", "cneg",
                                  "cnan", "cinf", "null"])
def test_set_robust_refuses(lib, case):
    rng = np.random.default_rng(2)
    g = _small_graph(lib, rng)
    target = 1
    g.set_robust(2, rm.HUBER, 3.0)
    kind, c, want = rm.CAUCHY, 1.0, -13
    if case == "foreign":
        # a factor of a type the library does not make: its eval is not the library's
        f = lib.dll.april_graph_factor_xyt_create(0, 1, (C.c_double * 3)(0, 0, 0), None, C.byref(g._matd(np.eye(3))))
        f.contents.type = 99
        f.contents.eval = g.factor(1).copy          # (any other function pointer)
        lib._add_factor(g.ptr, f)
        target, want = g.n_factors - 1, -12
    elif case == "max":
        target, want = g.add_factor_max(0, 1, [np.zeros(3)], [np.eye(3).reshape(9)], [0.0]), -12
    elif case == "max_of_robust":
        # a robust component: max_create refuses it (-12), the component stays with the caller
        comp = lib.dll.april_graph_factor_xyt_create(0, 1, (C.c_double * 3)(0, 0, 0), None, C.byref(g._matd(np.eye(3))))
        assert lib.dll.aprilsam_amd_factor_set_robust(comp, rm.CAUCHY, 1.0) == 0
        comps = (C.POINTER(abi.Factor) * 1)(comp)
        lib.clear_error()
        assert not lib.dll.aprilsam_amd_factor_max_create(comps, (C.c_double * 1)(0.0), 1)
        assert lib.last_error()[0] == -12
        abi.destroy_factor(comp)
        g.destroy()
        return
    elif case in ("asym", "indefinite"):
        Wd = g.factor(1).u.W.contents.data
        if case == "asym":
            Wd[1] += 1e-9
        else:
            Wd[0] = -abs(Wd[0])
        want = -12
    elif case == "kind_low":
        kind = -1
    elif case == "kind_high":
        kind = 4
    elif case == "c0":
        c = 0.0
    elif case == "cneg":
        c = -1.0
    elif case == "cnan":
        c = float("nan")
    elif case == "cinf":
        c = float("inf")
    if case == "null":
        lib.clear_error()
        assert lib.dll.aprilsam_amd_factor_set_robust(None, rm.CAUCHY, 1.0) == -13
        assert lib.last_error()[0] == -13
        g.destroy()
        return
    before = g.get_robust(target)
    lib.clear_error()
    assert g.set_robust(target, kind, c) == want
    assert lib.last_error()[0] == want
    assert g.get_robust(target) == before
    assert g.get_robust(2) == (rm.HUBER, 3.0)
    g.destroy()


def test_copy_is_deep(lib):
    g = _small_graph(lib, np.random.default_rng(3))
    for i in (0, 1):
        assert g.set_robust(i, rm.DCS, 2.0) == 0
        f = g.factor(i)
        cp = _COPY(f.copy)(C.cast(C.pointer(f), C.c_void_p))
        k, c = C.c_int(), C.c_double()
        lib.dll.aprilsam_amd_factor_get_robust(cp, C.byref(k), C.byref(c))
        assert (k.value, c.value) == (rm.DCS, 2.0)
        assert lib.dll.aprilsam_amd_factor_set_robust(cp, rm.HUBER, 5.0) == 0
        assert g.get_robust(i) == (rm.DCS, 2.0)          # the original keeps its loss
        abi.destroy_factor(cp)
        assert g.get_robust(i) == (rm.DCS, 2.0)
    g.destroy()


# ---- 3. host eval ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_host_eval_against_model(lib, kind):
    rng = np.random.default_rng(4 + kind)
    g = _small_graph(lib, rng, n=6)
    for n in range(g.n_nodes):           # l_point and state apart, so that eval and state_eval read different points
        g.set_state(n, g.states()[n] + rng.normal(0, 0.7, 3))
    states, fa, fb, z, W = g.arrays()
    lp, st = g.l_points(), g.states()
    c = 1.3
    plain_bits = {}
    for i in range(g.n_factors):
        f = g.factor(i)
        for which in (("eval", "state_eval") if fb[i] >= 0 else ("eval",)):
            e = _call_eval(f, g, which)
            plain_bits[(i, which)] = ([e.contents.r[k] for k in range(3)], [e.contents.W.contents.data[k] for k in range(9)], e.contents.chi2,
                                      [[e.contents.jacobians[j].contents.data[k] for k in range(9)] for j in range(1 + (fb[i] >= 0))])
            lib.dll.april_graph_factor_eval_destroy(C.cast(e, C.c_void_p))
        assert g.set_robust(i, kind, c) == 0
    for i in range(g.n_factors):
        f = g.factor(i)
        for which in (("eval", "state_eval") if fb[i] >= 0 else ("eval",)):
            P = lp if (which == "eval" and fb[i] >= 0) else st          # (xytpos eval reads the state, as the reference's)
            _, _, r = lm_model.linearise(P, fa[i:i + 1], fb[i:i + 1], z[i:i + 1])
            s = float(r[0] @ W[i].reshape(3, 3) @ r[0])
            w = float(rm.weight(kind, c, s))
            e = _call_eval(f, g, which)
            r0, W0, chi0, J0 = plain_bits[(i, which)]
            assert [e.contents.r[k] for k in range(3)] == r0                       # r and J unchanged, bitwise
            assert [[e.contents.jacobians[j].contents.data[k] for k in range(9)] for j in range(1 + (fb[i] >= 0))] == J0
            w0 = float(rm.weight(kind, c, chi0))          # (the weight of the library's own s: one multiply per entry)
            assert [e.contents.W.contents.data[k] for k in range(9)] == [w0 * v for v in W0]
            np.testing.assert_allclose(chi0, s, rtol=1e-12)
            np.testing.assert_allclose(e.contents.chi2, rm.rho(kind, c, chi0), rtol=1e-15)
            np.testing.assert_allclose(w, rm.weight(kind, c, chi0), rtol=1e-12)
            lib.dll.april_graph_factor_eval_destroy(C.cast(e, C.c_void_p))
    # NONE: the plain bits again
    for i in range(g.n_factors):
        assert g.set_robust(i, rm.NONE, 0) == 0
        e = _call_eval(g.factor(i), g, "eval")
        r0, W0, chi0, _ = plain_bits[(i, "eval")]
        assert [e.contents.r[k] for k in range(3)] == r0 and [e.contents.W.contents.data[k] for k in range(9)] == W0 and e.contents.chi2 == chi0
        lib.dll.april_graph_factor_eval_destroy(C.cast(e, C.c_void_p))
    g.destroy()


# ---- 4. saving ------------------------------------------------------------------------------------------------------------------
def test_save_refuses_a_robust_graph(lib, tmp_path):
    def make():
        return _small_graph(lib, np.random.default_rng(5))
    ref = make()
    p0 = str(tmp_path / "plain.graph")
    assert ref.save(p0) == 1
    g = make()
    assert g.set_robust(2, rm.CAUCHY, 1.0) == 0
    p1 = str(tmp_path / "robust.graph")
    assert g.save(p1) == 0 and not os.path.exists(p1)
    assert g.set_robust(2, rm.NONE, 0) == 0
    assert g.save(p1) == 1
    assert open(p0, "rb").read() == open(p1, "rb").read()
    ref.destroy(); g.destroy()


# ---- 5. the model against the unmodified reference ------------------------------------------------------------------------------
def _err(a, b):
    d = a - b
    return float(np.mean(np.hypot(d[:, 0], d[:, 1])))


@pytest.mark.parametrize("kind, c", [(rm.CAUCHY, 1.0), (rm.DCS, 3.0)])
def test_m3500_outliers_on_reference(reflib, tmp_path, kind, c):
    """M3500's loop closures and 50 false ones, all robust, 10 reference batch steps through the checker factor: the states follow the
    model's IRLS iteration, and end much closer to the outlier-free solution than the plain graph's.  Reference run, mean position error
    against the outlier-free solution: 37.4 m plain, 7.9 m with Cauchy c = 1, 9.2 m with DCS c = 3."""
    cl = rm.build_helper_lib(str(tmp_path))
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(kind, c)
    g = rm.build_checker(reflib, cl, states, plain, kinds, cs)
    p = reflib.new_param()
    xs = []
    for _ in range(10):
        g.cholesky(p)
        xs.append(g.states())
    p.destroy(); g.destroy()
    model = rm.irls_steps(states, plain, kinds, cs, 10)
    for k in range(10):
        np.testing.assert_allclose(xs[k], model[k], rtol=0, atol=1e-8)
    clean = tuple(np.asarray(v)[:nb + nl] for v in plain)
    xc = rm.irls_steps(states, clean, np.zeros(nb + nl, int), np.zeros(nb + nl), 10)[-1]
    xp = rm.irls_steps(states, plain, np.zeros(len(kinds), int), np.zeros(len(kinds)), 10)[-1]
    e_plain, e_rob = _err(xp, xc), _err(xs[-1], xc)
    assert e_plain > 30 and e_rob < 0.4 * e_plain, (e_rob, e_plain)


# ---- 6. the LM model ------------------------------------------------------------------------------------------------------------
def _random_graph(seed, n=30, extra=25):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0, 1, (n, 3)), axis=0)
    fa, fb, z, W = [0], [-1], [x[0] + rng.normal(0, 0.1, 3)], [np.diag([100.0, 100.0, 50.0]).reshape(9)]
    pairs = [(i, i + 1) for i in range(n - 1)] + [tuple(sorted(rng.choice(n, 2, replace=False))) for _ in range(extra)]
    for a, b in pairs:
        zz = mm.residual(x[a], x[b], np.zeros(3)) * -1 + rng.normal(0, 0.3, 3)
        if rng.random() < 0.2:
            zz = rng.normal(0, 5, 3)          # outliers
        fa.append(a); fb.append(b); z.append(zz); W.append(np.diag(rng.uniform(2, 30, 3)).reshape(9))
    plain = (np.array(fa), np.array(fb), np.array(z), np.array(W))
    kinds = rng.integers(0, 4, len(fa)); cs = rng.uniform(0.5, 3, len(fa))
    return lm_model.perturbed(x + rng.normal(0, 0.3, x.shape), 0.2, seed), plain, kinds, cs


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_lm_model_pred_and_monotone_on_random_graphs(seed):
    x0, plain, kinds, cs = _random_graph(seed)
    out = rm.optimize(x0, plain, kinds, cs, max_iters=30)
    for pred, hB, hh, lam in out["preds"]:
        np.testing.assert_allclose(pred, hB + lam * hh, rtol=1e-9, atol=1e-12 * abs(hB))
    Fs = [out["F_initial"]] + [row[0] for row in out["trace"] if row[3] == 1]
    assert all(b <= a for a, b in zip(Fs, Fs[1:]))
    assert out["accepted"] > 0 and out["F_final"] < out["F_initial"]


def test_lm_model_on_m3500_outliers():
    """Cauchy LM on M3500 with 50 false closures ends much closer to the outlier-free solution than plain LM (model figures: the
    numbers the GPU test asserts)"""
    states, plain, kinds, cs, nb, nl = rm.m3500_robust(rm.CAUCHY, 1.0)
    out = rm.optimize(states, plain, kinds, cs, max_iters=30)
    for pred, hB, hh, lam in out["preds"]:
        np.testing.assert_allclose(pred, hB + lam * hh, rtol=1e-8)
    Fs = [out["F_initial"]] + [row[0] for row in out["trace"] if row[3] == 1]
    assert all(b <= a for a, b in zip(Fs, Fs[1:]))
    clean = tuple(np.asarray(v)[:nb + nl] for v in plain)
    xc = lm_model.optimize(states, clean, max_iters=30)["x"]
    xp = lm_model.optimize(states, plain, max_iters=30)["x"]
    e_rob, e_plain = _err(out["x"], xc), _err(xp, xc)
    assert e_rob < 0.4 * e_plain, (e_rob, e_plain)
