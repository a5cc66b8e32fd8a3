"""Range / bearing / range-bearing factors, host side: the constructor's layout, deep copies, destroy and every
refusal; the library's host eval / state_eval against the numpy model and central differences; aprilsam_amd_debug_polar_slot -- the
formulas host and kernels share -- against the model's true m-row factors; the refusals of set_robust, max_create and save; the solver
entry points without a device.  No GPU."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from aprilsam_amd import abi
from tests.conftest import ROOT
from tests.support import polar_model as pm
from tests.support.normal_eq import linearise

KINDS = (pm.RANGE, pm.BEARING, pm.RANGE_BEARING)


class Matd(C.Structure):
    _fields_ = [("nrows", C.c_uint), ("ncols", C.c_uint)]


class Eval(C.Structure):
    _fields_ = [("chi2", C.c_double), ("jacobians", C.POINTER(C.c_void_p)), ("length", C.c_int), ("r", C.POINTER(C.c_double)), ("W", C.c_void_p)]


_EVAL = C.CFUNCTYPE(C.POINTER(Eval), C.c_void_p, C.c_void_p, C.c_void_p)
_COPY = C.CFUNCTYPE(C.POINTER(abi.Factor), C.c_void_p)


def _matd(addr):
    m = Matd.from_address(addr)
    n = m.nrows * m.ncols
    return np.array((C.c_double * n).from_address(addr + C.sizeof(Matd))).reshape(m.nrows, m.ncols)


def _eval(lib, f, g, which):
    e = _EVAL(getattr(f, which))(C.cast(C.pointer(f), C.c_void_p), C.cast(g.ptr, C.c_void_p), None)
    ev = e.contents
    out = dict(chi2=ev.chi2, length=ev.length, Ja=_matd(ev.jacobians[0]), Jb=_matd(ev.jacobians[1]), end=ev.jacobians[2],
               r=np.array([ev.r[k] for k in range(ev.length)]), W=_matd(ev.W))
    lib.dll.april_graph_factor_eval_destroy.argtypes = [C.c_void_p]
    lib.dll.april_graph_factor_eval_destroy(C.cast(e, C.c_void_p))
    return out


def _random_case(rng, kind):
    m = pm.rows(kind)
    M = rng.normal(size=(m, m))
    W = M @ M.T + np.diag(rng.uniform(1, 2000, m))
    W = 0.5 * (W + W.T)
    z = np.array([rng.uniform(0.05, 8.0), rng.uniform(-np.pi, np.pi)])
    z = z[:1] if kind == pm.RANGE else z[1:] if kind == pm.BEARING else z
    return z.copy(), W


def _graph(lib, rng, kind, z, W, n=3):
    g = lib.new_graph()
    for _ in range(n):
        g.add_node_xyt(rng.normal(0, 3, 3))
    g.add_factor_xytpos(0, [0, 0, 0], np.eye(3))
    i = g.add_factor_polar(kind, 2, 1, z, W)
    return g, i


# ---- 1. the object ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_layout_copy_destroy(lib, kind):
    rng = np.random.default_rng(10 + kind)
    z, W = _random_case(rng, kind)
    g, i = _graph(lib, rng, kind, z, W)
    m = pm.rows(kind)
    f = g.factor(i)
    assert f.type == abi.FACTOR_POLAR_TYPE == 4 and f.nnodes == 2 and f.length == m
    assert (f.nodes[0], f.nodes[1]) == (2, 1)
    assert [f.u.z[k] for k in range(m)] == list(z) and not f.u.ztruth
    Wm = _matd(C.cast(f.u.W, C.c_void_p).value)
    assert Wm.shape == (m, m) and np.array_equal(Wm, W)
    assert g.get_polar(i) == kind and g.get_polar(0) == 0
    assert lib.dll.aprilsam_amd_factor_get_polar(None, None) == 0
    assert g.get_robust(i) == (abi.ROBUST_NONE, 0.0)
    # copy is deep: same content, own storage, survives the original's edit; destroy through the factor's own pointer
    c = _COPY(f.copy)(C.cast(C.pointer(f), C.c_void_p))
    cf = c.contents
    assert cf.type == 4 and cf.length == m and (cf.nodes[0], cf.nodes[1]) == (2, 1)
    assert C.addressof(cf.u.z.contents) != C.addressof(f.u.z.contents) and C.cast(cf.u.W, C.c_void_p).value != C.cast(f.u.W, C.c_void_p).value
    assert cf.u.impl != f.u.impl and cf.eval == f.eval and cf.state_eval == f.state_eval and cf.destroy == f.destroy
    f.u.z[0] = 123.0
    assert cf.u.z[0] == z[0]
    k = C.c_int(-1)
    lib.dll.aprilsam_amd_factor_get_polar(c, C.byref(k))
    assert k.value == kind
    abi.destroy_factor(c)
    g.destroy()


@pytest.mark.parametrize("case", ["kind0", "kind4", "self", "z_nan", "z_inf", "w_zero", "w_neg", "w_nan", "w_inf", "w_asym", "w_indef", "null_z", "null_w"])
def test_create_refuses(lib, case):
    kind, a, b = pm.RANGE_BEARING, 0, 1
    z, W = np.array([1.0, 0.2]), np.array([[4.0, 1.0], [1.0, 9.0]])
    want = -13
    if case == "kind0": kind = 0
    elif case == "kind4": kind = 4
    elif case == "self": b = 0
    elif case == "z_nan": z[1] = np.nan
    elif case == "z_inf": kind, z = pm.RANGE, np.array([np.inf, 0.0])
    elif case == "w_zero": kind, W, want = pm.BEARING, np.array([[0.0, 0], [0, 0]]), -12
    elif case == "w_neg": kind, W, want = pm.RANGE, np.array([[-1.0, 0], [0, 0]]), -12
    elif case == "w_nan": W[1, 1], want = np.nan, -12
    elif case == "w_inf": W[0, 0], want = np.inf, -12
    elif case == "w_asym": W[0, 1], want = np.nextafter(1.0, 2.0), -12
    elif case == "w_indef": W, want = np.array([[1.0, 2.0], [2.0, 1.0]]), -12
    zz = None if case == "null_z" else np.ascontiguousarray(z).ctypes.data_as(C.POINTER(C.c_double))
    WW = None if case == "null_w" else np.ascontiguousarray(W).ctypes.data_as(C.POINTER(C.c_double))
    lib.clear_error()
    f = lib.dll.aprilsam_amd_factor_polar_create(kind, a, b, zz, WW)
    assert not f
    code, msg = lib.last_error()
    assert code == want and "aprilsam_amd_factor_polar_create" in msg, (code, msg)


def test_other_constructs_refuse_polar_factors(lib, tmp_path):
    rng = np.random.default_rng(3)
    g, i = _graph(lib, rng, pm.RANGE_BEARING, [1.0, 0.1], np.diag([4.0, 9.0]))
    # a loss on a polar factor
    lib.clear_error()
    assert g.set_robust(i, abi.ROBUST_HUBER, 1.0) == -12 and lib.last_error()[0] == -12
    assert g.get_robust(i) == (abi.ROBUST_NONE, 0.0) and g.get_polar(i) == pm.RANGE_BEARING
    # a polar factor as a max component: refused, the component stays with the caller
    comp = g.make_factor_polar(pm.RANGE, 0, 1, [1.0], [2.0])
    arr = (C.POINTER(abi.Factor) * 1)(comp)
    lib.clear_error()
    assert not lib.dll.aprilsam_amd_factor_max_create(arr, np.zeros(1).ctypes.data_as(C.POINTER(C.c_double)), 1)
    assert lib.last_error()[0] == -12
    abi.destroy_factor(comp)
    # .graph files cannot hold them
    path = tmp_path / "polar.graph"
    assert g.save(str(path)) is False and not path.exists()
    g.destroy()


# ---- 2. eval / state_eval ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_eval_against_model_and_central_differences(lib, kind):
    rng = np.random.default_rng(20 + kind)
    for trial in range(20):
        z, W = _random_case(rng, kind)
        g, i = _graph(lib, rng, kind, z, W)
        for n in range(3):          # l_point != state: eval reads the former, state_eval the latter
            g.set_state(n, g.states_of(n) + rng.normal(0, 0.3, 3))
        pol = (kind, 2, 1, z, W)
        for which, x in (("eval", g.l_points()), ("state_eval", g.states())):
            e = _eval(lib, g.factor(i), g, which)
            Ja, Jb, r, Wm = pm.evaluate(x, pol)
            m = pm.rows(kind)
            assert e["length"] == m and e["Ja"].shape == (m, 3) == e["Jb"].shape and e["W"].shape == (m, m) and not e["end"]
            assert np.array_equal(e["W"], W)
            scale = max(1.0, np.abs(Ja).max())
            assert np.abs(e["Ja"] - Ja).max() <= 1e-13 * scale and np.abs(e["Jb"] - Jb).max() <= 1e-13 * scale
            assert np.abs(e["r"] - r).max() <= 1e-13 * max(1.0, np.abs(r).max())
            assert abs(e["chi2"] - r @ W @ r) <= 1e-12 * max(1.0, r @ W @ r)
            # central differences of the MODEL's residual (a step of 1e-6 rho: see tests/test_polar_model.py)
            rho = np.hypot(*pm.rel(x[2], x[1])[0])
            eps = 1e-6 * min(1.0, rho)
            for node, J in ((2, e["Ja"]), (1, e["Jb"])):
                for k in range(3):
                    xp, xm = x.copy(), x.copy()
                    xp[node, k] += eps; xm[node, k] -= eps
                    d = pm.evaluate(xp, pol)[2] - pm.evaluate(xm, pol)[2]
                    if kind != pm.RANGE:
                        d[-1] = pm.mod2pi(d[-1])
                    assert np.abs(-d / (2 * eps) - J[:, k]).max() <= 1e-7 * scale
        g.destroy()


# ---- 3. the slot ----------------------------------------------------------------------------------------------------------------
def _slot_case(rng, kind, special):
    pa = rng.normal(0, 3, 3); pb = rng.normal(0, 3, 3)
    z, W = _random_case(rng, kind)
    if special == "wrap":            # b almost straight behind a, the measured bearing on the other side of +-pi
        pb[:2] = pa[:2] + np.array([np.cos(pa[2] + np.pi - 1e-3), np.sin(pa[2] + np.pi - 1e-3)]) * rng.uniform(0.5, 4)
        if kind != pm.RANGE:
            z[-1] = -np.pi + 2e-3
    elif special == "tiny":          # rho of 1e-8
        th = rng.uniform(-np.pi, np.pi)
        pb[:2] = pa[:2] + 1e-8 * np.array([np.cos(th), np.sin(th)])
        if kind != pm.BEARING:
            z[0] = 2e-8
    return pa, pb, z, W


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("special", ["random", "wrap", "tiny"])
def test_slot_reproduces_the_m_row_factor(lib, kind, special):
    rng = np.random.default_rng(100 * kind + len(special))
    worst = worst_m = 0.0
    for _ in range(300 if special == "random" else 40):
        pa, pb, z, W = _slot_case(rng, kind, special)
        ze, We = lib.polar_slot(kind, pa, pb, z, W)
        assert np.array_equal(We, We.T) and np.all(We[2] == 0) and np.all(We[:, 2] == 0)          # bitwise symmetric, zero theta row
        x = np.vstack([pa, pb])
        Jxa, Jxb, rx = linearise(x, [0], [1], ze[None])            # the xyt factor the slot describes, at the same point
        Jx = np.hstack([Jxa[0], Jxb[0]])
        assert rx[0, 2] == 0.0                                     # z_eff's theta component is the predicted one
        Ja, Jb, r, Wp = pm.evaluate(x, (kind, 0, 1, z, W))
        Jp = np.hstack([Ja, Jb])
        if special == "wrap" and kind != pm.RANGE:
            assert abs(r[-1]) < 0.01                               # (wrapped: not 2 pi away)
        H, Hp = Jx.T @ We @ Jx, Jp.T @ Wp @ Jp
        b, bp = Jx.T @ We @ rx[0], Jp.T @ Wp @ r
        worst = max(worst, np.abs(H - Hp).max() / np.abs(Hp).max(), np.abs(b - bp).max() / max(np.abs(bp).max(), 1e-300))
        # LM's model decrease read from the slot
        h = rng.normal(0, 1e-3 * min(1.0, np.hypot(*pm.rel(pa, pb)[0])), 6)
        d, dp = Jx @ h, Jp @ h
        m, mp = d @ We @ (2 * rx[0] - d), dp @ Wp @ (2 * r - dp)
        # the two terms may cancel: relative to their sizes.  z_eff - q returns r_eff with an absolute error of 2 ulp of the larger of
        # |q| and |z_eff| per component, which d' W_eff multiplies by 2: that much is allowed on top
        ulp = 4 * np.finfo(float).eps * max(np.abs(ze[:2]).max(), np.abs(ze[:2] - rx[0, :2]).max())
        worst_m = max(worst_m, (abs(m - mp) - 2 * np.abs(We @ d).sum() * ulp) / (abs(dp @ Wp @ (2 * r)) + abs(dp @ Wp @ dp)))
    print(f"kind {kind} {special}: worst relative deviation of H and b {worst:.3e}, of the model decrease {worst_m:.3e}")
    assert worst <= 1e-12, worst
    assert worst_m <= 1e-12, worst_m


@pytest.mark.parametrize("kind", KINDS)
def test_zero_range_gives_a_null_slot(lib, kind):
    rng = np.random.default_rng(kind)
    z, W = _random_case(rng, kind)
    pa = np.array([1.5, -2.0, 0.7]); pb = np.array([1.5, -2.0, -0.4])
    ze, We = lib.polar_slot(kind, pa, pb, z, W)
    assert np.all(We == 0) and np.all(np.isfinite(ze))
    assert np.array_equal(ze, [0.0, 0.0, pb[2] - pa[2]])
    # a non-finite input propagates
    ze, We = lib.polar_slot(kind, [np.nan, 0, 0], [1, 1, 0], z, W)
    assert np.isnan(ze[:2]).all() and np.isnan(We[:2, :2]).all()
    with pytest.raises(ValueError):
        lib.polar_slot(7, pa, pb, z, W)


# ---- 4. without a device ------------------------------------------------------------------------------------------------------
CODE = r"""
import sys; sys.path.insert(0, %r)
import numpy as np
from aprilsam_amd import host
from tests.support import polar_model as pm
l = host.SolverLib()
d = pm.snake(4, 3, seed=0)
g = pm.build(l, d["start"], d["plain"], d["polars"]); p = l.new_param()
before = g.states()
l.clear_error(); g.cholesky(p); assert l.last_error()[0] == -14, l.last_error()
l.clear_error(); assert np.isnan(g.chi2()) and l.last_error()[0] == -14
l.clear_error(); assert l.dll.aprilsam_amd_resident_begin(g.ptr, p.ptr) == -14 and l.last_error()[0] == -14
try:
    g.optimize_lm(p)
except host.LMError as e:
    assert e.code == -14, e.code
else:
    raise AssertionError("no error")
assert np.array_equal(g.states(), before)
print("RETURNED")
"""


def test_solver_entry_points_refuse_without_a_device(lib):
    if lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    r = subprocess.run([sys.executable, "-c", CODE % ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RETURNED" in r.stdout, (r.stdout, r.stderr)
