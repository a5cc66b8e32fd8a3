"""Max-mixture factors on the host: the constructor's u.max layout and argument checks, copy / destroy, the
library's host eval / state_eval against the numpy model (tests/support/maxmix_model.py), and the outlier scenario on the
unmodified reference driving the independent checker factor (tests/support/maxmix_factor.c).  No GPU."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import abi
from tests.support import maxmix_model as mm


class Eval(C.Structure):
    _fields_ = [("chi2", C.c_double), ("jacobians", C.POINTER(C.POINTER(abi.Matd3x3))), ("length", C.c_int),
                ("r", C.POINTER(C.c_double)), ("W", C.POINTER(abi.Matd3x3))]


_EVAL = C.CFUNCTYPE(C.POINTER(Eval), C.c_void_p, C.c_void_p, C.c_void_p)
_COPY = C.CFUNCTYPE(C.POINTER(abi.Factor), C.c_void_p)


def _call_eval(f, g, which):
    fn = _EVAL(getattr(f.contents, which))
    return fn(C.cast(f, C.c_void_p), C.cast(g.ptr, C.c_void_p), None)


def _comps(rng, K, spread=1.0):
    zs = rng.normal(0, spread, (K, 3))
    Ws = []
    for _ in range(K):
        M = rng.normal(size=(3, 3))
        Ws.append((M @ M.T + np.diag(rng.uniform(1, 50, 3))).reshape(9))
    return zs, np.array(Ws), rng.normal(0, 1, K)


def test_layout_of_u_max(lib):
    g = lib.new_graph()
    for i in range(3):
        g.add_node_xyt([i, 0.1 * i, 0.0])
    zs, Ws, lw = _comps(np.random.default_rng(1), 3)
    f = g.make_factor_max(0, 2, zs, Ws, lw)
    assert f.contents.type == abi.FACTOR_MAX_TYPE == 3
    assert f.contents.nnodes == 2 and (f.contents.nodes[0], f.contents.nodes[1]) == (0, 2)
    v = abi.max_view(f)
    assert v.nfactors == 3
    assert [v.logw[i] for i in range(3)] == list(lw)
    for i in range(3):
        c = v.factors[i].contents
        assert c.type == 1 and (c.nodes[0], c.nodes[1]) == (0, 2)
        assert [c.u.z[k] for k in range(3)] == list(zs[i])
        assert [c.u.W.contents.data[k] for k in range(9)] == list(Ws[i])
    lib._add_factor(g.ptr, f)            # the graph owns it now: destroy frees the components too
    assert g.n_factors == 1
    g.destroy()


@pytest.mark.parametrize("case", ["k0", "k9", "pair", "asym", "det", "logw"])
def test_constructor_refuses(lib, case):
    g = lib.new_graph()
    for i in range(3):
        g.add_node_xyt([i, 0, 0])
    rng = np.random.default_rng(2)
    K = {"k0": 0, "k9": 9}.get(case, 2)
    zs, Ws, lw = _comps(rng, max(K, 1))
    zs, Ws, lw = zs[:K], Ws[:K], lw[:K]
    if case == "asym":
        Ws[1][1] += 0.5
    if case == "det":
        Ws[0] = -Ws[0]
    if case == "logw":
        lw[1] = np.inf
    if case == "pair":
        comps = (C.POINTER(abi.Factor) * 2)()
        for i, (a, b) in enumerate([(0, 1), (0, 2)]):
            m = g._matd(Ws[i])
            comps[i] = lib.dll.april_graph_factor_xyt_create(a, b, (C.c_double * 3)(*zs[i]), None, C.byref(m))
        lib.clear_error()
        assert not lib.dll.aprilsam_amd_factor_max_create(comps, (C.c_double * 2)(*lw), 2)
        assert lib.last_error()[0] == -12
        for i in range(2):
            abi.destroy_factor(comps[i])
    else:
        lib.clear_error()
        with pytest.raises(ValueError):
            g.make_factor_max(0, 1, zs, Ws, lw)
        assert lib.last_error()[0] == -12
    g.destroy()


def test_copy_and_destroy(lib):
    g = lib.new_graph()
    for i in range(2):
        g.add_node_xyt([i, 0, 0])
    zs, Ws, lw = _comps(np.random.default_rng(3), 4)
    f = g.make_factor_max(0, 1, zs, Ws, lw)
    c = _COPY(f.contents.copy)(C.cast(f, C.c_void_p))
    assert c.contents.type == 3 and c.contents.eval == f.contents.eval
    vf, vc = abi.max_view(f), abi.max_view(c)
    assert vc.nfactors == 4 and C.addressof(vc.logw.contents) != C.addressof(vf.logw.contents)
    for i in range(4):
        a, b = vf.factors[i].contents, vc.factors[i].contents
        assert C.addressof(a) != C.addressof(b)
        assert [b.u.z[k] for k in range(3)] == list(zs[i]) and [b.u.W.contents.data[k] for k in range(9)] == list(Ws[i])
        assert vc.logw[i] == lw[i]
    abi.destroy_factor(f)                # the copy does not share anything with the original
    assert [abi.max_view(c).factors[3].contents.u.z[k] for k in range(3)] == list(zs[3])
    abi.destroy_factor(c)
    g.destroy()


def test_host_eval_against_model(lib):
    rng = np.random.default_rng(4)
    g = lib.new_graph()
    N = 6
    for i in range(N):
        g.add_node_xyt(rng.normal(0, 2, 3))
    picked = set()
    for trial in range(40):
        a, b = (int(v) for v in rng.choice(N, 2, replace=False))
        K = int(rng.integers(1, 9))
        zs, Ws, lw = _comps(rng, K, spread=2.0)
        f = g.make_factor_max(a, b, zs, Ws, lw)
        lib._add_factor(g.ptr, f)
        # l_point and state apart, so that eval and state_eval read different points
        for n in (a, b):
            g.set_state(n, rng.normal(0, 2, 3), relinearize=True)
            g.set_state(n, g.states()[n] + rng.normal(0, 0.5, 3))
        lp, st = g.l_points(), g.states()
        for which, P in (("eval", lp), ("state_eval", st)):
            s = mm.select(P[a], P[b], zs, Ws, lw)
            picked.add(s)
            e = _call_eval(f, g, which)
            r = mm.residual(P[a], P[b], zs[s])
            np.testing.assert_allclose([e.contents.r[k] for k in range(3)], r, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(e.contents.chi2, mm.rtwr(Ws[s], r), rtol=1e-12)
            assert [e.contents.W.contents.data[k] for k in range(9)] == list(Ws[s])
            lib.dll.april_graph_factor_eval_destroy(C.cast(e, C.c_void_p))
    assert len(picked) > 3                # (the scenario exercises more than the first component)
    g.destroy()


def test_selection_rule_ties_and_nan():
    z = np.zeros(3); W = np.eye(3).reshape(9)
    assert mm.select(np.zeros(3), np.ones(3), [z, z, z], [W, W, W], [0.0, 0.0, 0.0]) == 0          # tie: lower index
    assert mm.select(np.zeros(3), np.ones(3), [z, z], [W, W], [np.nan, 5.0]) == 0                    # NaN s_0 keeps component 0
    assert mm.select(np.zeros(3), np.ones(3), [z, z, z], [W, W, W], [0.0, np.nan, 1.0]) == 2


def test_m3500_outliers_on_reference(reflib, tmp_path):
    """The scenario the GPU tests replay: M3500's loop closures as 2-component max factors and 50 false loop closures of the same
    form.  10 reference batch iterations through the checker factor end much closer to the outlier-free solution than the same
    graph with the outliers as plain xyt factors; no selection is a near-tie; selections change between iterations."""
    cl = mm.build_helper_lib(str(tmp_path))
    states, base, loops, outl = mm.m3500_outliers()

    def run(edges, as_max, rec=None):
        g = mm.build(reflib, states, base, edges, as_max, mm.helper_adder(reflib, cl, 99, rec) if as_max else None)
        p = reflib.new_param()
        out, sels = [], []
        for _ in range(10):
            g.cholesky(p)
            out.append(g.states())
            if rec is not None:
                sels.append(np.array([cl.mm_last(f) for f in rec]))
        p.destroy(); g.destroy()
        return out, sels

    def err(a, b):
        d = a - b
        return float(np.mean(np.hypot(d[:, 0], d[:, 1])))

    clean, _ = run(loops, False)
    plain, _ = run(loops + outl, False)
    cl.mm_reset_stats()
    rec = []
    mixed, sels = run(loops + outl, True, rec)
    e_plain, e_mixed = err(plain[-1], clean[-1]), err(mixed[-1], clean[-1])
    # reference run: 37.4 (outliers as plain factors) against 14.6 (as max factors), mean position error in m
    assert e_mixed < 0.5 * e_plain, (e_mixed, e_plain)
    assert np.all(sels[-1][-len(outl):] == 1)          # every false loop closure ends on its null hypothesis
    assert cl.mm_min_margin() > 1e-6, cl.mm_min_margin()
    assert any(np.any(sels[i] != sels[i - 1]) for i in range(1, len(sels)))
