"""Polar gates, host side: aprilsam_amd_debug_polar_gate -- the function host and kernels share -- against the numpy
model (tests/support/polar_gate_model.py); what aprilsam_amd_gate_polar / aprilsam_amd_associate_polar refuse before any device is asked
for; both calls without a device.  No GPU."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from aprilsam_amd import host
from tests.conftest import ROOT
from tests.support import polar_gate_model as pg
from tests.support import polar_model as pm

KINDS = (pm.RANGE, pm.BEARING, pm.RANGE_BEARING)


def _case(rng, kind, wrap=False):
    """poses 0.5 to 8 m apart, a measurement a few sigma off the prediction (wrap: the bearing 2 pi k away, and b behind a, where atan2
    jumps), W and the joint covariance C symmetric positive definite"""
    m = pm.rows(kind)
    pa = rng.normal(0, [3, 3, 2])
    t = rng.uniform(-np.pi, np.pi)
    if wrap:
        t = pa[2] + np.pi + rng.normal(0, 1e-3)
    pb = np.r_[pa[:2] + rng.uniform(0.5, 8.0) * np.array([np.cos(t), np.sin(t)]), rng.uniform(-np.pi, np.pi)]
    q = pm.rel(pa, pb)[0]
    zz = pm.h(pm.RANGE_BEARING, q) + rng.normal(0, [0.1, 0.05])
    if wrap:
        zz[1] += 2 * np.pi * rng.integers(-2, 3)
    z = zz[:1] if kind == pm.RANGE else zz[1:] if kind == pm.BEARING else zz
    M = rng.normal(size=(m, m))
    W = M @ M.T + np.diag(rng.uniform(50, 500, m)); W = 0.5 * (W + W.T)
    M = rng.normal(size=(6, 6))
    Cc = 1e-3 * (M @ M.T + 6 * np.eye(6)); Cc = 0.5 * (Cc + Cc.T)
    return pa, pb, z, W, Cc


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("special", ["random", "wrap"])
def test_debug_gate_against_the_model(lib, kind, special):
    rng = np.random.default_rng(10 * kind + len(special))
    worst = 0.0
    for _ in range(300 if special == "random" else 60):
        pa, pb, z, W, Cc = _case(rng, kind, special == "wrap")
        ok, d2, S = lib.polar_gate(kind, pa, pb, z, W, Cc)
        mok, md2, mS = pg.gate_one(kind, z, W, pa, pb, Cc)
        assert ok and mok and np.array_equal(S, S.T)               # bitwise symmetric
        if special == "wrap" and kind != pm.RANGE:
            assert md2 < 200                                      # (wrapped: a residual 2 pi away would give d2 of 10^4)
        worst = max(worst, np.abs(S - mS).max() / np.abs(mS).max(), abs(d2 - md2) / max(1.0, md2))
    print(f"kind {kind} {special}: aprilsam_amd_debug_polar_gate against the model, worst {worst:.3e}")
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("kind", KINDS)
def test_zero_range_heading_and_padding(lib, kind):
    rng = np.random.default_rng(kind)
    pa, pb, z, W, Cc = _case(rng, kind)
    m = pm.rows(kind)
    # rho == 0: not ok, NaN
    ok, d2, S = lib.polar_gate(kind, pa, np.r_[pa[:2], 0.3], z, W, Cc)
    assert not ok and np.isnan(d2) and np.isnan(S).all()
    # b's heading, and the row and column of C that belong to it, change nothing -- bitwise
    ok, d2, S = lib.polar_gate(kind, pa, pb, z, W, Cc)
    pb2 = pb.copy(); pb2[2] += 1.234
    C2 = Cc.copy(); C2[5, :] = np.nan; C2[:, 5] = np.nan
    ok2, d22, S2 = lib.polar_gate(kind, pa, pb2, z, W, C2)
    assert ok and ok2 and d2 == d22 and S.tobytes() == S2.tobytes()
    # the raw call: a 1-row kind reads z[0] and W[0] only and writes S4[0] with zeros behind it
    zz = np.full(2, np.nan); zz[:m] = z
    WW = np.full(4, np.nan); WW[:m * m] = W.ravel()
    d2r = C.c_double(-7.0); S4 = np.full(4, -7.0)
    rc = lib.dll.aprilsam_amd_debug_polar_gate(kind, host._np_d(pa), host._np_d(pb), host._np_d(zz), host._np_d(WW), host._np_d(Cc.reshape(36).copy()),
                                               C.byref(d2r), host._np_d(S4))
    assert rc == 0 and d2r.value == d2 and np.array_equal(S4[:m * m].reshape(m, m), S) and np.all(S4[m * m:] == 0)
    with pytest.raises(ValueError):
        lib.polar_gate(7, pa, pb, z, W, Cc)
    lib.clear_error()
    assert lib.dll.aprilsam_amd_debug_polar_gate(kind, None, host._np_d(pb), host._np_d(zz), host._np_d(WW), host._np_d(Cc.reshape(36).copy()),
                                                 C.byref(d2r), host._np_d(S4)) == -13 and lib.last_error()[0] == -13


def _calls(lib, g, p):
    """(name, call(**changes) -> (rc, outputs untouched)) for the two entry points on valid arguments; a change replaces one argument"""
    ip, dp = host._np_i, host._np_d
    i32 = lambda v: np.ascontiguousarray(v, np.int32)

    def gate(**ch):
        a = dict(g=g.ptr, p=p.ptr, n=2, a=i32([0, 1]), b=i32([2, 3]), kind=i32([pm.RANGE, pm.RANGE_BEARING]), z=np.array([1.0, np.nan, 1.2, 0.3]),
                 W=np.array([4.0, np.nan, np.nan, np.nan, 5.0, 1.0, 1.0, 6.0]), d2=np.full(2, -7.0), S=np.full(8, -7.0))
        a.update(ch)
        ptr = lambda v, f: None if v is None else f(v)
        rc = lib.dll.aprilsam_amd_gate_polar(a["g"], a["p"], a["n"], ptr(a["a"], ip), ptr(a["b"], ip), ptr(a["kind"], ip), ptr(a["z"], dp), ptr(a["W"], dp),
                                             ptr(a["d2"], dp), ptr(a["S"], dp))
        return rc, all(np.all(a[k] == -7.0) for k in ("d2", "S") if a[k] is not None)

    def assoc(**ch):
        a = dict(g=g.ptr, p=p.ptr, observer=0, m=2, kind=i32([pm.BEARING, pm.RANGE_BEARING]), z=np.array([0.1, np.nan, 1.2, 0.3]),
                 W=np.array([4.0, np.nan, np.nan, np.nan, 5.0, 1.0, 1.0, 6.0]), L=3, lm=i32([1, 2, 3]), g1=pg.CHI2_1_999, g2=pg.CHI2_2_999,
                 d2=np.full(6, -7.0), best=np.full(2, -7, np.int32), d2b=np.full(2, -7.0), d2s=np.full(2, -7.0))
        a.update(ch)
        ptr = lambda v, f: None if v is None else f(v)
        rc = lib.dll.aprilsam_amd_associate_polar(a["g"], a["p"], a["observer"], a["m"], ptr(a["kind"], ip), ptr(a["z"], dp), ptr(a["W"], dp), a["L"], ptr(a["lm"], ip),
                                                  a["g1"], a["g2"], ptr(a["d2"], dp), ptr(a["best"], ip), ptr(a["d2b"], dp), ptr(a["d2s"], dp))
        return rc, all(np.all(a[k] == -7) for k in ("d2", "best", "d2b", "d2s") if a[k] is not None)
    return gate, assoc


def _four_nodes(lib):
    g = lib.new_graph()
    for k in range(4):
        g.add_node_xyt([float(k), 0.5 * k, 0.1 * k])
    return g, lib.new_param()


REFUSALS_GATE = [
    (dict(a=None), -13), (dict(kind=None), -13), (dict(z=None), -13), (dict(W=None), -13), (dict(d2=None), -13), (dict(n=-1), -13),
    (dict(kind=np.array([0, 3], np.int32)), -13), (dict(kind=np.array([1, 4], np.int32)), -13),
    (dict(b=np.array([2, 1], np.int32)), -13),                                                       # a == b
    (dict(z=np.array([np.inf, 0.0, 1.2, 0.3])), -13), (dict(z=np.array([1.0, 0.0, 1.2, np.nan])), -13),
    (dict(W=np.array([4.0, 0, 0, 0, 5.0, np.nan, 1.0, 6.0])), -13),
    (dict(W=np.array([-4.0, 0, 0, 0, 5.0, 1.0, 1.0, 6.0])), -12),                                    # w <= 0
    (dict(W=np.array([4.0, 0, 0, 0, 5.0, 1.0, 1.5, 6.0])), -12),                                     # asymmetric
    (dict(W=np.array([4.0, 0, 0, 0, 1.0, 3.0, 3.0, 1.0])), -12),                                     # indefinite
]
REFUSALS_ASSOC = [
    (dict(kind=None), -13), (dict(lm=None), -13), (dict(best=None), -13), (dict(d2b=None), -13), (dict(d2s=None), -13), (dict(m=-1), -13), (dict(L=-2), -13),
    (dict(kind=np.array([2, 9], np.int32)), -13),
    (dict(lm=np.array([1, 0, 3], np.int32)), -13),                                                    # the observer among the landmarks
    (dict(g1=np.nan), -13), (dict(g2=np.inf), -13),
    (dict(z=np.array([np.nan, 0.0, 1.2, 0.3])), -13),
    (dict(W=np.array([4.0, 0, 0, 0, 5.0, 1.0, 1.0, -6.0])), -12),
]


def test_refusals_come_before_the_device(lib):
    """what needs neither graph contents nor factor is refused at once: the same codes with and without a device, nothing written; the
    entries a 1-row kind does not read may hold anything (NaN here)"""
    g, p = _four_nodes(lib)
    gate, assoc = _calls(lib, g, p)
    for ch, code in REFUSALS_GATE:
        lib.clear_error()
        assert gate(**ch) == (code, True) and lib.last_error()[0] == code, ch
    for ch, code in REFUSALS_ASSOC:
        lib.clear_error()
        assert assoc(**ch) == (code, True) and lib.last_error()[0] == code, ch
    lib.clear_error()
    want = -1 if lib.device_count() > 0 else -14                    # valid arguments: no retained factor / no device -- the unread NaN entries pass
    assert gate() == (want, True) and assoc() == (want, True) and assoc(d2=None) == (want, True)
    p.destroy(); g.destroy()


CODE = r"""
import sys; sys.path.insert(0, %r)
import numpy as np
from aprilsam_amd import host
from tests.test_polar_gate_host import _calls, _four_nodes, REFUSALS_GATE, REFUSALS_ASSOC
l = host.SolverLib()
assert l.device_count() == 0
g, p = _four_nodes(l)
gate, assoc = _calls(l, g, p)
for ch, code in REFUSALS_GATE:
    assert gate(**ch) == (code, True), ch
for ch, code in REFUSALS_ASSOC:
    assert assoc(**ch) == (code, True), ch
l.clear_error(); assert gate() == (-14, True) and l.last_error()[0] == -14, l.last_error()
l.clear_error(); assert assoc() == (-14, True) and l.last_error()[0] == -14, l.last_error()
assert gate(n=0) == (-14, True) and assoc(m=0) == (-14, True)
print("RETURNED")
"""


def test_entry_points_refuse_without_a_device(lib):
    if lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    r = subprocess.run([sys.executable, "-c", CODE % ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RETURNED" in r.stdout, (r.stdout, r.stderr)
