"""Dense Gaussian factors and aprilsam_amd_graph_remove_nodes, host side: the constructor's layout, deep copies,
destroy and every refusal with its code; the library's host eval / state_eval -- the square-root form R, d of the diagonally pivoted
Cholesky -- against the numpy model (tests/support/marginal_prior_model.py): J'J = Lambda, J'r = eta - Lambda delta, chi2 = c0 - 2 eta'delta
+ delta'Lambda delta, each to ten times what the float64 model deviates from the longdouble model on the same input (DESIGN.md section 24
records the figures); in-place edits; the refusals of set_robust, max_create and save; remove_nodes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import abi
from tests.support import marginal_prior_model as mm
from tests.support.gaussian_graphs import random_gaussian as _case


class Matd(C.Structure):
    _fields_ = [("nrows", C.c_uint), ("ncols", C.c_uint)]


class Eval(C.Structure):
    _fields_ = [("chi2", C.c_double), ("jacobians", C.POINTER(C.c_void_p)), ("length", C.c_int), ("r", C.POINTER(C.c_double)), ("W", C.c_void_p)]


_EVAL = C.CFUNCTYPE(C.POINTER(Eval), C.c_void_p, C.c_void_p, C.c_void_p)
_COPY = C.CFUNCTYPE(C.POINTER(abi.Factor), C.c_void_p)


def _matd(addr):
    m = Matd.from_address(addr)
    n = m.nrows * m.ncols
    return np.array((C.c_double * n).from_address(addr + C.sizeof(Matd)), float).reshape(m.nrows, m.ncols)


def _eval(lib, f, g, which):
    """dict(chi2, length, J [length, 3k], r, W, end): one evaluation through the factor's own pointer, freed by the library's eval_destroy"""
    e = _EVAL(getattr(f, which))(C.cast(C.pointer(f), C.c_void_p), C.cast(g.ptr, C.c_void_p), None)
    ev = e.contents
    k = f.nnodes
    out = dict(chi2=ev.chi2, length=ev.length, J=np.hstack([_matd(ev.jacobians[i]) for i in range(k)]), end=ev.jacobians[k],
               r=np.array([ev.r[i] for i in range(ev.length)]), W=_matd(ev.W))
    lib.dll.april_graph_factor_eval_destroy.argtypes = [C.c_void_p]
    lib.dll.april_graph_factor_eval_destroy(C.cast(e, C.c_void_p))
    return out


def _graph(lib, rng, nodes, xbar, eta, Lam, n=6):
    g = lib.new_graph()
    for _ in range(n):
        g.add_node_xyt(rng.normal(0, 2, 3))
    g.add_factor_xytpos(0, [0, 0, 0], np.eye(3))
    return g, g.add_factor_gaussian(nodes, xbar, eta, Lam)


# ---- 1. the object ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,name,rank", [(1, "regular", 3), (2, "regular", 6), (2, "relative", 3), (2, "zero", 0), (3, "relative", 6), (11, "regular", 33)])
def test_layout_copy_destroy(lib, k, name, rank):
    rng = np.random.default_rng(100 + k)
    xbar, eta, Lam = _case(rng, name, k)
    nodes = list(rng.permutation(11)[:k])
    g, i = _graph(lib, rng, nodes, xbar, eta, Lam, n=11)
    f = g.factor(i)
    assert f.type == abi.FACTOR_GAUSSIAN_TYPE == 5 and f.nnodes == k and f.length == rank
    assert [f.nodes[j] for j in range(k)] == nodes and not f.u.ztruth
    assert [f.u.z[j] for j in range(6 * k)] == list(xbar.ravel()) + list(eta)
    Wm = _matd(C.cast(f.u.W, C.c_void_p).value)
    assert Wm.shape == (3 * k, 3 * k) and np.array_equal(Wm, Lam)
    assert g.get_gaussian(i) == k and g.get_gaussian(0) == 0 and g.get_polar(i) == 0
    assert lib.dll.aprilsam_amd_factor_get_gaussian(None, None) == 0
    c = _COPY(f.copy)(C.cast(C.pointer(f), C.c_void_p))
    cf = c.contents
    assert cf.type == 5 and cf.nnodes == k and cf.length == rank and [cf.nodes[j] for j in range(k)] == nodes
    assert C.addressof(cf.u.z.contents) != C.addressof(f.u.z.contents) and C.cast(cf.u.W, C.c_void_p).value != C.cast(f.u.W, C.c_void_p).value
    assert C.addressof(cf.nodes.contents) != C.addressof(f.nodes.contents)
    assert cf.u.impl != f.u.impl and cf.eval == f.eval and cf.state_eval == f.state_eval and cf.destroy == f.destroy and cf.copy == f.copy
    f.u.z[0] = 123.0                                               # the copy survives the original's edit
    assert cf.u.z[0] == xbar[0, 0]
    kk = C.c_int(-1)
    lib.dll.aprilsam_amd_factor_get_gaussian(c, C.byref(kk))
    assert kk.value == k
    a, b = _eval(lib, f, g, "eval"), _eval(lib, cf, g, "eval")     # (xbar[0] differs: the residuals do, the Jacobians do not)
    assert np.array_equal(a["J"], b["J"]) and a["length"] == b["length"] == rank
    abi.destroy_factor(c)
    g.destroy()


@pytest.mark.parametrize("case", ["k0", "k12", "dup", "xbar_nan", "eta_inf", "L_nan", "L_inf", "L_asym", "L_indef", "L_negdiag", "L_zero_diag_offdiag",
                                  "null_nodes", "null_xbar", "null_eta", "null_L"])
def test_create_refuses(lib, case):
    k = 2
    rng = np.random.default_rng(1)
    xbar, eta, Lam = _case(rng, "regular", 12 if case == "k12" else k)
    nodes = np.arange(12 if case == "k12" else k, dtype=np.int32)
    want = -13
    if case == "k0": k = 0
    elif case == "k12": k, want = 12, -12
    elif case == "dup": nodes[1] = nodes[0]
    elif case == "xbar_nan": xbar[1, 2] = np.nan
    elif case == "eta_inf": eta[3] = np.inf
    elif case == "L_nan": Lam[2, 2], want = np.nan, -12
    elif case == "L_inf": Lam[0, 0], want = np.inf, -12
    elif case == "L_asym": Lam[0, 1], want = np.nextafter(Lam[0, 1], np.inf), -12
    elif case == "L_indef": Lam, want = np.diag([1.0, 1, 1, 1, 1, 1]), -12; Lam[0, 1] = Lam[1, 0] = 2.0
    elif case == "L_negdiag": Lam, want = np.diag([1.0, 1, -1e-3, 1, 1, 1]), -12
    elif case == "L_zero_diag_offdiag": Lam, want = np.zeros((6, 6)), -12; Lam[0, 1] = Lam[1, 0] = 1.0
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    args = [None if case == "null_nodes" else np.ascontiguousarray(nodes).ctypes.data_as(ip),
            None if case == "null_xbar" else np.ascontiguousarray(xbar).ctypes.data_as(dp),
            None if case == "null_eta" else np.ascontiguousarray(eta).ctypes.data_as(dp),
            None if case == "null_L" else np.ascontiguousarray(Lam).ctypes.data_as(dp)]
    lib.clear_error()
    f = lib.dll.aprilsam_amd_factor_gaussian_create(k, *args)
    assert not f
    code, msg = lib.last_error()
    assert code == want and "aprilsam_amd_factor_gaussian_create" in msg, (code, msg)


def test_other_families_refuse_a_gaussian_factor(lib, tmp_path):
    rng = np.random.default_rng(2)
    g, i = _graph(lib, rng, [1, 2], *_case(rng, "regular", 2))
    lib.clear_error()
    assert g.set_robust(i, abi.ROBUST_HUBER, 1.0) == -12 and lib.last_error()[0] == -12            # a robust loss on it
    comps = (C.POINTER(abi.Factor) * 1)(g.factor_ptr(i))
    lw = np.zeros(1)
    lib.clear_error()
    assert not lib.dll.aprilsam_amd_factor_max_create(comps, lw.ctypes.data_as(C.POINTER(C.c_double)), 1)  # as a max component
    assert lib.last_error()[0] == -12
    assert g.save(str(tmp_path / "g.graph")) is False and not (tmp_path / "g.graph").exists()        # .graph files cannot hold it
    g.destroy()


# ---- 2. eval / state_eval against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,name", [(2, "regular"), (2, "relative"), (2, "zero"), (1, "regular"), (3, "relative"), (11, "regular"), (11, "relative")])
def test_eval_is_the_square_root_form(lib, k, name):
    rng = np.random.default_rng(200 + 7 * k + len(name))
    xbar, eta, Lam = _case(rng, name, k)
    nodes = [int(v) for v in rng.permutation(11)[:k]]
    g, i = _graph(lib, rng, nodes, xbar, eta, Lam, n=11)
    for j, nd in enumerate(nodes):                                 # l_points near xbar, states elsewhere; one heading across the wrap
        g.set_state(nd, xbar[j] + rng.normal(0, 0.1, 3), relinearize=True)
        g.set_state(nd, xbar[j] + rng.normal(0, 0.3, 3))
    f = g.factor(i)
    n = 3 * k
    R64, d64, c64 = mm.sqrt_form(eta, Lam, np.float64)
    Rl, dl, cl = mm.sqrt_form(eta, Lam, np.longdouble)
    assert len(R64) == len(Rl) == f.length
    for which, pts in (("eval", g.l_points()), ("state_eval", g.states())):
        ev = _eval(lib, f, g, which)
        L = ev["length"]
        assert L == f.length and ev["J"].shape == (L, n) and ev["r"].shape == (L,) and not ev["end"]
        assert np.array_equal(ev["W"], np.eye(L))
        ref, dev = {}, {}
        for tag, R, d, c0, dt in (("f64", R64, d64, c64, np.float64), ("ld", Rl, dl, cl, np.longdouble)):
            delta = mm.gaussian_delta(pts, nodes, xbar, dt)
            r = d - R @ delta
            ref[tag] = dict(JtJ=R.T @ R, Jtr=R.T @ r, chi2=r @ r,
                            g=np.asarray(eta, dt) - np.asarray(Lam, dt) @ delta, q=mm.gaussian_chi2(pts, nodes, xbar, eta, Lam, c0, dt))
        J = ev["J"].astype(np.longdouble); r = ev["r"].astype(np.longdouble)
        got = dict(JtJ=J.T @ J, Jtr=J.T @ r, chi2=np.longdouble(ev["chi2"]))
        for key in ("JtJ", "Jtr", "chi2"):
            allowed = 10 * float(np.max(np.abs(ref["f64"][key] - ref["ld"][key]), initial=0.0))
            err = float(np.max(np.abs(got[key] - ref["ld"][key]), initial=0.0))
            print(f"gaussian host {which} k={k} {name} {key}: |library - longdouble| = {err:.3e}, allowed 10 x |float64 - longdouble| = {allowed:.3e}")
            assert err <= allowed, (which, key, err, allowed)
        # ... and the square-root form IS the information form (the model, longdouble): J'J = Lambda, J'r = eta - Lambda delta, chi2 = c0 - ...
        scale = max(1.0, float(np.max(np.abs(Lam))))
        assert float(np.max(np.abs(ref["ld"]["JtJ"] - Lam), initial=0.0)) < 1e-13 * scale
        assert float(np.max(np.abs(ref["ld"]["Jtr"] - ref["ld"]["g"]), initial=0.0)) < 1e-11 * scale
        assert abs(float(ref["ld"]["chi2"] - ref["ld"]["q"])) < 1e-11 * max(1.0, float(ref["ld"]["q"])) and ev["chi2"] >= 0
    g.destroy()


def test_edit_in_place_factorises_again(lib):
    rng = np.random.default_rng(3)
    xbar, eta, Lam = _case(rng, "regular", 2)
    g, i = _graph(lib, rng, [2, 4], xbar, eta, Lam)
    f = g.factor(i)
    a = _eval(lib, f, g, "eval")
    f.u.z[6] += 0.5                                                # eta[0]
    b = _eval(lib, f, g, "eval")
    assert np.array_equal(a["J"], b["J"]) and not np.array_equal(a["r"], b["r"])
    eta2 = eta.copy(); eta2[0] += 0.5
    R, d, _ = mm.sqrt_form(eta2, Lam)
    assert np.allclose(b["J"].T @ b["r"], eta2 - Lam @ mm.gaussian_delta(g.l_points(), [2, 4], xbar), rtol=0, atol=1e-9 * np.max(np.abs(Lam)))
    Wp = C.cast(C.cast(f.u.W, C.c_void_p).value + C.sizeof(Matd), C.POINTER(C.c_double))
    Wp[1] = Wp[1] + 1.0                                            # no longer symmetric: the evaluation is refused, not wrong
    e = _EVAL(f.eval)(C.cast(C.pointer(f), C.c_void_p), C.cast(g.ptr, C.c_void_p), None)
    assert not e
    Wp[1] = Wp[1] - 1.0
    c = _eval(lib, f, g, "eval")
    assert np.array_equal(c["J"], b["J"]) and np.array_equal(c["r"], b["r"])
    g.destroy()


# ---- 3. aprilsam_amd_graph_remove_nodes ---------------------------------------------------------------------------------------------
def _edit_graph(lib):
    g = lib.new_graph()
    for i in range(8):
        g.add_node_xyt([float(i), 0.1 * i, 0.01 * i])
    g.add_factor_xytpos(0, [0, 0, 0], np.eye(3))                                                    # 0
    for i in range(7):
        g.add_factor_xyt(i, i + 1, [1.0, 0.1, 0.01], np.eye(3))                                     # 1 .. 7
    g.add_factor_max(1, 6, [[5, 0.5, 0.05], [0, 0, 0]], [np.eye(3).ravel(), 1e-3 * np.eye(3).ravel()], [0.0, -2.0])   # 8
    g.add_factor_max(2, 3, [[1, 0.1, 0.01], [0, 0, 0]], [np.eye(3).ravel(), 1e-3 * np.eye(3).ravel()], [0.0, -2.0])   # 9: touches node 3
    g.add_factor_polar(abi.POLAR_RANGE, 7, 5, [2.0], [4.0])                                         # 10
    rng = np.random.default_rng(4)
    g.add_factor_gaussian([6, 0, 4], *_case(rng, "relative", 3))                                    # 11
    g.add_factor_gaussian([5, 3], *_case(rng, "regular", 2))                                        # 12: touches node 3
    return g


def _snapshot(g):
    nodes = [C.addressof(g.node(i)) for i in range(g.n_nodes)]
    facs = [(C.addressof(g.factor(i)), [g.factor(i).nodes[k] for k in range(g.factor(i).nnodes)]) for i in range(g.n_factors)]
    return nodes, facs


def test_remove_nodes_renumbers_and_keeps_the_order(lib):
    g = _edit_graph(lib)
    nodes0, facs0 = _snapshot(g)
    states0 = g.states()
    idx = g.remove_nodes([3, 2])
    assert list(idx) == [0, 1, -1, -1, 2, 3, 4, 5]
    assert g.n_nodes == 6 and np.array_equal(g.states(), states0[[0, 1, 4, 5, 6, 7]])
    nodes1, facs1 = _snapshot(g)
    assert nodes1 == [nodes0[i] for i in (0, 1, 4, 5, 6, 7)]                                        # the surviving objects, in order
    kept = [i for i, (_, nn) in enumerate(facs0) if not ({2, 3} & set(nn))]
    assert kept == [0, 1, 5, 6, 7, 8, 10, 11]
    assert [a for a, _ in facs1] == [facs0[i][0] for i in kept]
    assert [nn for _, nn in facs1] == [[int(idx[x]) for x in facs0[i][1]] for i in kept]
    mx = abi.max_view(g.factor(5))                                                                   # old factor 8: max on (1, 6) -> (1, 4)
    assert mx.nfactors == 2
    for j in range(2):
        cf = mx.factors[j].contents
        assert (cf.nodes[0], cf.nodes[1]) == (1, 4)
    assert g.get_gaussian(7) == 3 and [g.factor(7).nodes[k] for k in range(3)] == [4, 0, 2]
    assert list(g.remove_nodes([])) == list(range(6)) and g.n_nodes == 6                            # m = 0: the identity
    g.destroy()


@pytest.mark.parametrize("remove,word", [([8], "out of range"), ([-1], "out of range"), ([2, 5, 2], "twice")])
def test_remove_nodes_refusal_leaves_every_pointer_in_place(lib, remove, word):
    g = _edit_graph(lib)
    before = _snapshot(g)
    lib.clear_error()
    with pytest.raises(ValueError) as e:
        g.remove_nodes(remove)
    assert word in str(e.value) and lib.last_error()[0] == -13
    assert _snapshot(g) == before and g.n_nodes == 8 and g.n_factors == 13
    g.factor(4).nodes[1] = 99                                      # a factor that names a node outside the graph
    with pytest.raises(ValueError):
        g.remove_nodes([0])
    g.factor(4).nodes[1] = 4
    assert _snapshot(g) == before
    idx = np.full(8, 7, np.int32)
    assert lib.dll.aprilsam_amd_graph_remove_nodes(None, 0, None, None) == -13
    assert lib.dll.aprilsam_amd_graph_remove_nodes(g.ptr, 1, None, idx.ctypes.data_as(C.POINTER(C.c_int))) == -13 and (idx == 7).all()
    g.destroy()
