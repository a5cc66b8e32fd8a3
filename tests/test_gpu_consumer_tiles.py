"""The retained-factor consumers at every size at which their shared tile bodies change form (selinv.hip.h: tile_trsm, sel_wave,
sel_tile_store, sel_mma; pathsolve.hip.h: xyt_joint_cov): the 16-row tile SEL_T, an exact multiple of it, and the 64-deep k chunk of
sel_mma.  The graphs are the designed clique trees of tests/support/clique_trees.py, whose plans tests/test_clique_tree_plans.py
pins front by front, so a front's s and u are known: CASES below says what each one puts on which side of which size.

Per case, against the dense system at g.l_points() (built as tests/test_gpu_treesolve.py::_system builds it):
  solve          three modes, nrhs in (1, 15, 16, 17, 33) -- a column tile that is partial, full, full + 1, two + 1 -- and the identity.
                 FULL: backward error < OMEGA_LIMIT, forward error < SIG_RTOL.  Forward / backward of the identity: F'F and B B' against
                 the dense inverse at SIG_RTOL (tests/test_gpu_treesolve.py::test_modes), and of the other right-hand sides against those
                 two matrices applied on the CPU.  FULL == backward(forward) and chunked (solve_chunk_cols = 16) == unchunked, bit for bit.
  covariances    marginals, marginals_joint of every factor pair, marginals_joint_any of all pairs among the first 5, 6, 11 and 16 poses of
                 the first leaf (15, 18, 33 and 48 columns through one front, where the leaf has that many poses) and of random pairs:
                 check_blocks / check_any at SIG_RTOL.
  anchors        marginals_cross (SIG_RTOL) and relative_covariances (GATE_RTOL) to an anchor in a leaf and to one in the root.
  gate           twelve candidates against tests/support/gate_model.py at GATE_RTOL.
Every call is made twice: same bits.

All tolerances are the project's constants, imported.  The cases are anchored (clique_trees.ORDER_DEV = 5e-15 on their dx); every test
prints what two CPU references of the same solve (numpy's dense solve, scipy's splu with another elimination order) differ by, in the
units of the forward-error check: at most 6.9e-15 over all cases (1.5e-15 and 3.4e-15 on the two largest, the 425-pose and the
190-pose tree), five orders of magnitude inside SIG_RTOL.  Observed on an MI355X over all cases: backward error <= 1.6e-15, forward
error <= 7.1e-15, every covariance, anchor and gate figure below 1e-14 (DESIGN.md section 28 has the scratch mutations this file was
seen to catch)."""
import numpy as np
import pytest

from aprilsam_amd.host import MarginalsError
from tests.support import clique_trees as CT
from tests.support.gate_model import gate, gate_inputs
from tests.support.marginal_cases import factor_pairs
from tests.support.selinv_model import sparse_system, system_blocks
from tests.support.sigma_compare import SIG_RTOL, check_any, check_blocks, random_pairs, row_scale
from tests.support.treesolve_model import OMEGA_LIMIT, backward_error, relative_covariances, rhs_columns
from tests.test_gpu_treesolve import GATE_RTOL

pytestmark = pytest.mark.gpu

CASES = {
    "clique 1": "s = 3, a single pose",
    "clique 5": "s = 15: below one tile",
    "clique 6": "s = 18: above one tile, i0 > 0 first taken",
    "clique 16": "s = 48: three full tiles, no partial one",
    "clique 21": "s = 63: the k loop of the solve's product ends inside one 64 chunk",
    "clique 22": "s = 66: ... past one 64 chunk",
    "clique 43": "s = 129: two chunks and a rest",
    "6,5 x2": "u = 15 against s = 18",
    "11,10 x2": "u = 30, s = 33",
    "22,21 x2": "leaves s = 66, u = 63",
    "23,22 x2": "leaves s = 69, u = 66: gemmt's k range past 64",
    "5 x4 deep, fan 4": "many tiny fronts, four levels of gathers",
    "30,25,20 fan 2": "unequal s on a level: the longest-first order of the solve entries",
}
NRHS = (1, 15, 16, 17, 33)
MODES = ("full", "forward", "backward")
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for arr, g, p, A, Sig, scale in _CACHE.values():
        p.destroy(); g.destroy()
    _CACHE.clear()


def _twice(f):
    """f() made twice: the same bits both times"""
    a, b = f(), f()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert x.tobytes() == y.tobytes()
    return a


def _case(lib, name):
    """(arrays, graph, param, A sparse, Sigma, row scales) after one batch step; built once per case and only read afterwards"""
    if name not in _CACHE:
        levels, fan, _, _ = CT.CASES[name]
        arr = CT.clique_tree(levels, fan, CT.SEED)
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
        states, fa, fb, z, W = g.arrays()
        Aii, Aab = system_blocks(g.l_points(), fa, fb, z, W, p.c.tikhanov, None)
        A = sparse_system(Aii, Aab, fa, fb).tocsc()
        Sig = np.linalg.inv(A.toarray())
        Sig.setflags(write=False)
        _CACHE[name] = (arr, g, p, A, Sig, row_scale(Sig))
    return _CACHE[name]


def _forward_error(X, ref):
    """per column |X - ref| / max |ref| (|X| where the reference column is zero); X, ref: [3N, ncol]"""
    scale = np.abs(ref).max(axis=0)
    return np.where(scale > 0, np.abs(X - ref).max(axis=0) / np.where(scale > 0, scale, 1.0), np.abs(X).max(axis=0))


@pytest.mark.parametrize("name", list(CASES))
def test_solves(lib, name):
    import scipy.sparse.linalg as sla
    arr, g, p, A, Sig, scale = _case(lib, name)
    N = len(arr[0])
    rs = np.repeat(scale, 3)[:, None]
    I = np.eye(3 * N)
    Fw = _twice(lambda: g.solve(p, I, "forward")).T              # columns: L^-1 e_j (permuted back)
    Bw = _twice(lambda: g.solve(p, I, "backward")).T
    eF, eB = (np.abs(Fw.T @ Fw - Sig) / rs).max(), (np.abs(Bw @ Bw.T - Sig) / rs).max()
    print(f"[tiles] {name} ({CASES[name]}): F'F {eF:.2e}, B B' {eB:.2e} of Sigma's row scale")
    assert eF < SIG_RTOL and eB < SIG_RTOL, (name, eF, eB)
    Ad = A.toarray()
    lu = sla.splu(A, permc_spec="MMD_AT_PLUS_A")
    for nrhs in NRHS:
        B = np.ascontiguousarray(rhs_columns(N, nrhs, 100 + nrhs).T)
        X = {m: _twice(lambda m=m: g.solve(p, B, m)) for m in MODES}
        ref = np.linalg.solve(Ad, B.T)
        cpu = _forward_error(lu.solve(B.T), ref).max()
        w, fe = backward_error(A, X["full"].T, B.T).max(), _forward_error(X["full"].T, ref).max()
        ff, fb_ = _forward_error(X["forward"].T, Fw @ B.T).max(), _forward_error(X["backward"].T, Bw @ B.T).max()
        print(f"[tiles] {name} nrhs {nrhs}: omega {w:.2e}, forward error {fe:.2e} (two CPU solves differ by {cpu:.2e}), "
              f"forward / backward against the identity's {ff:.2e} / {fb_:.2e}")
        assert X["full"].shape == B.shape and all(np.isfinite(x).all() for x in X.values())
        assert w < OMEGA_LIMIT, (name, nrhs, w)
        assert fe < SIG_RTOL and ff < SIG_RTOL and fb_ < SIG_RTOL, (name, nrhs, fe, ff, fb_)
        assert g.solve(p, X["forward"], "backward").tobytes() == X["full"].tobytes(), (name, nrhs)
        if nrhs > 2:
            assert np.all(X["full"][2] == 0.0)                   # the zero column
        with lib.options(solve_chunk_cols=16):
            for m in MODES:
                assert g.solve(p, B, m).tobytes() == X[m].tobytes(), (name, nrhs, m)


@pytest.mark.parametrize("name", list(CASES))
def test_covariances(lib, name):
    arr, g, p, A, Sig, scale = _case(lib, name)
    states, fa, fb, z, W = arr
    N = len(states)
    ref = (Sig, scale)
    pa, pb = factor_pairs(fa, fb)
    d = _twice(lambda: g.marginals(p))
    j = _twice(lambda: g.marginals_joint(p, pa, pb)) if len(pa) else None
    worst = dict(blocks=check_blocks(ref, fa, fb, d, j))
    leaf = CT.layout(*CT.CASES[name][:2])[0][1]                  # poses of the first leaf: 0 .. leaf - 1
    for k in (5, 6, 11, 16):                                     # 3 k columns through the leaf's front
        if k <= leaf:
            a, b = (v.astype(np.int32) for v in np.triu_indices(k, 1))
            worst[f"any {3 * k} cols"] = check_any(ref, a, b, _twice(lambda: g.marginals_joint_any(p, a, b)))
    a, b = random_pairs(N, 1, 40)                                # both orders and a == b, all over the tree
    worst["any random"] = check_any(ref, a, b, _twice(lambda: g.marginals_joint_any(p, a, b)))
    print(f"[tiles] {name} ({CASES[name]}): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("name", list(CASES))
def test_anchors_and_gate(lib, name):
    arr, g, p, A, Sig, scale = _case(lib, name)
    N = len(arr[0])
    x = g.states()
    nodes = np.arange(N)
    Sii = np.stack([Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in nodes])
    for anchor in sorted({0, N - 1}):                            # a pose of the first leaf, a pose of the root
        Cx = _twice(lambda: g.marginals_cross(p, anchor))
        Sia = Sig[:, 3 * anchor:3 * anchor + 3].reshape(N, 3, 3)
        ec = (np.abs(Cx - Sia).reshape(N, 9).max(axis=1) / np.maximum(scale, scale[anchor])).max()
        assert ec < SIG_RTOL, (name, anchor, ec)
        R = _twice(lambda: g.relative_covariances(p, anchor))
        model = relative_covariances(x, anchor, nodes, Sii[anchor], Sii, Sia)
        assert np.all(R[anchor] == 0.0)
        others = nodes[nodes != anchor]
        er = 0.0
        if len(others):
            er = (np.abs(R[others] - model[others]).max(axis=(1, 2)) / np.abs(model[others]).max(axis=(1, 2))).max()
            assert er < GATE_RTOL, (name, anchor, er)
        print(f"[tiles] {name} anchor {anchor}: cross {ec:.2e}, relative {er:.2e}")
    if N == 1:                                                   # (the one candidate there is joins the pose to itself: refused)
        with pytest.raises(MarginalsError) as e:
            g.gate_xyt(p, [0], [0], np.zeros((1, 3)), np.eye(3).reshape(1, 9))
        assert e.value.code == -13
        return
    ga, gb, gz, gW = gate_inputs(arr, 12, 5)
    d2, S = _twice(lambda: g.gate_xyt(p, ga, gb, gz, gW))
    J = g.marginals_joint_any(p, ga, gb)
    check_any((Sig, scale), ga, gb, J)
    md2, mS = gate(x, ga, gb, gz, gW, J)
    ed, eS = (np.abs(d2 - md2) / np.abs(md2)).max(), np.abs(S - mS).max() / np.abs(mS).max()
    print(f"[tiles] {name} gate: d2 {ed:.2e}, S {eS:.2e}")
    assert (np.abs(d2 - md2) <= GATE_RTOL * np.abs(md2) + 1e-300).all() and eS < GATE_RTOL, (name, ed, eS)
