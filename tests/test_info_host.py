"""aprilsam_amd_logdet / aprilsam_amd_logdet_sets / aprilsam_amd_info_gain_xyt on the host side: the symbols are
exported and bound, every argument fault that needs neither graph contents nor device is refused at once with its code, the error is
recorded and the sentinel-filled outputs stay untouched; a well-formed call meets no retained factor (-1) on a machine with a device and
-14 on one without (there is no CPU fallback).  Runs without a GPU."""
import ctypes as C

import numpy as np

from aprilsam_amd import abi, datasets

SENT = -7.0
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
W0 = np.diag([100.0, 100.0, 400.0]).ravel()
SYMBOLS = ("aprilsam_amd_logdet", "aprilsam_amd_logdet_sets", "aprilsam_amd_info_gain_xyt")


def _d(x):
    return None if x is None else x.ctypes.data_as(_dp)


def _i(x):
    return None if x is None else x.ctypes.data_as(_ip)


def _graph(lib):
    g = lib.new_graph(); g.build_from_arrays(*datasets.random_pose_graph(40, 10, 0)); p = lib.new_param()
    return g, p


def _sets(lib, g, p, ptr=(0, 2, 3), nodes=(4, 9, 1), n_sets=None, null=()):
    """(rc, outputs untouched and the code recorded)"""
    ptr = np.asarray(ptr, np.int32); nodes = np.asarray(nodes, np.int32)
    out = np.full(len(nodes) + 2, SENT)
    a = dict(g=g.ptr, p=p.ptr, ptr=_i(ptr), nodes=_i(nodes), out=_d(out))
    for k in null:
        a[k] = None
    lib.clear_error()
    rc = lib.dll.aprilsam_amd_logdet_sets(a["g"], a["p"], len(ptr) - 1 if n_sets is None else n_sets, a["ptr"], a["nodes"], a["out"])
    return rc, bool(np.all(out == SENT)) and lib.last_error()[0] == rc


def _gain(lib, g, p, ptr=(0, 2, 3), a=(4, 9, 1), b=(7, 4, 30), W=None, n_hyp=None, null=()):
    ptr = np.asarray(ptr, np.int32); a = np.asarray(a, np.int32); b = np.asarray(b, np.int32)
    W = np.tile(W0, (len(a), 1)) if W is None else np.ascontiguousarray(W, float)
    out = np.full(len(a) + 2, SENT)
    v = dict(g=g.ptr, p=p.ptr, ptr=_i(ptr), a=_i(a), b=_i(b), W=_d(W), out=_d(out))
    for k in null:
        v[k] = None
    lib.clear_error()
    rc = lib.dll.aprilsam_amd_info_gain_xyt(v["g"], v["p"], len(ptr) - 1 if n_hyp is None else n_hyp, v["ptr"], v["a"], v["b"], v["W"], v["out"])
    return rc, bool(np.all(out == SENT)) and lib.last_error()[0] == rc


def _w(i, M):
    W = np.tile(W0, (3, 1)); W[i] = np.asarray(M, float).ravel()
    return W


def test_the_three_symbols_are_exported_and_bound(lib):
    for nm in SYMBOLS:
        assert hasattr(lib.dll, nm), nm
        assert getattr(lib.dll, nm).argtypes is not None, nm
    assert abi.SET_MAX == 16 == abi.JOINT_MAX
    g, _ = _graph(lib)
    for nm in ("logdet", "logdet_sets", "info_gain_xyt"):
        assert callable(getattr(g, nm)), nm
    g.destroy()


REFUSALS_SETS = [
    (dict(null=("g",)), -13), (dict(null=("p",)), -13), (dict(null=("ptr",)), -13), (dict(null=("nodes",)), -13), (dict(null=("out",)), -13),
    (dict(n_sets=-1), -13),
    (dict(ptr=(1, 2, 3)), -13),                                  # set_ptr[0] != 0
    (dict(ptr=(0, 2, 1)), -13),                                  # decreasing
    (dict(ptr=(0, 2, 2, 3)), -13),                               # an empty set
    (dict(ptr=(0, 17), nodes=np.arange(17)), -13),               # 17 nodes
    (dict(ptr=(0, 3), nodes=(4, 9, 4)), -13),                    # a node twice in a set
]
REFUSALS_GAIN = [
    (dict(null=("g",)), -13), (dict(null=("p",)), -13), (dict(null=("ptr",)), -13), (dict(null=("a",)), -13), (dict(null=("b",)), -13),
    (dict(null=("W",)), -13), (dict(null=("out",)), -13), (dict(n_hyp=-1), -13),
    (dict(ptr=(1, 2, 3)), -13), (dict(ptr=(0, 2, 1)), -13), (dict(ptr=(0, 2, 2, 3)), -13),
    (dict(ptr=(0, 17), a=np.arange(17), b=np.arange(17) + 20), -13),
    (dict(b=(7, 9, 30)), -13),                                   # a == b
    (dict(W=_w(1, [[1, 0, 0], [0, np.nan, 0], [0, 0, 1]])), -13), (dict(W=_w(2, [[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]])), -13),
    (dict(W=_w(0, np.diag([1.0, -1.0, 1.0]))), -12),             # indefinite
    (dict(W=_w(1, [[4, 1, 0], [1.5, 5, 0], [0, 0, 6]])), -12),   # asymmetric
    (dict(W=_w(2, [[1, 3, 0], [3, 1, 0], [0, 0, 1]])), -12),     # not positive definite
]


def test_argument_refusals_come_before_the_device_and_write_nothing(lib):
    g, p = _graph(lib)
    for ch, code in REFUSALS_SETS:
        assert _sets(lib, g, p, **ch) == (code, True), ch
    for ch, code in REFUSALS_GAIN:
        assert _gain(lib, g, p, **ch) == (code, True), ch
    out = np.full(2, SENT)
    lib.clear_error()
    assert lib.dll.aprilsam_amd_logdet(g.ptr, None, _d(out)) == -13 and lib.last_error()[0] == -13 and np.all(out == SENT)
    lib.clear_error()
    assert lib.dll.aprilsam_amd_logdet(g.ptr, p.ptr, None) == -13 and lib.last_error()[0] == -13
    p.destroy(); g.destroy()


def test_well_formed_calls_meet_no_factor_or_no_device(lib):
    """valid arguments on a param that was never solved: -14 without a device, -1 with one; nothing written either way"""
    from aprilsam_amd.host import MarginalsError
    want = -1 if lib.device_count() > 0 else -14
    g, p = _graph(lib)
    assert _sets(lib, g, p) == (want, True) and _sets(lib, g, p, ptr=(0, 16), nodes=np.arange(16)) == (want, True)
    assert _sets(lib, g, p, ptr=(0,), nodes=(0,)) == (want, True)                         # n_sets == 0 is admitted first
    assert _gain(lib, g, p) == (want, True) and _gain(lib, g, p, ptr=(0, 16), a=np.arange(16), b=np.arange(16) + 20) == (want, True)
    assert _gain(lib, g, p, a=(4, 9, 9), b=(7, 4, 4)) == (want, True)                     # a repeated pair is allowed
    out = np.full(2, SENT)
    lib.clear_error()
    assert lib.dll.aprilsam_amd_logdet(g.ptr, p.ptr, _d(out)) == want and lib.last_error()[0] == want and np.all(out == SENT)
    for call in (lambda: g.logdet(p), lambda: g.logdet_sets(p, [[0, 1], [2]]), lambda: g.info_gain_xyt(p, [([0, 1], [2, 3], np.tile(W0, (2, 1)))])):
        try:
            call()
        except MarginalsError as e:
            assert e.code == want
        else:
            raise AssertionError("no error")
    p.destroy(); g.destroy()
