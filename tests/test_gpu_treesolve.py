"""Solves with the retained factor on the GPU (aprilsam_amd_solve, aprilsam_amd_marginals_cross, aprilsam_amd_relative_covariances:
aprilsam_amd/csrc/treesolve.hip.h), checked on the CPU.

Two error measures:
  backward error   omega = max_i |A X - B|_i / (|A| |X| + |B|)_i per column, A from selinv_model.system_blocks / sparse_system at
                   g.l_points() with the param's tikhanov on the right nodes.  Limit OMEGA_LIMIT = 1e-12: scipy's splu (COLAMD and MMD)
                   reaches 1.6e-15 on M3500 and random0..3, so the limit leaves about 600 x for other summation orders, while a lost
                   block or a wrong row leaves omega at 1e-3 .. 1.  On the lattices splu itself reaches 1.499e-14 (K = 60, the 17
                   columns used here) and 1.896e-14 (K = 316, 3 columns) -- tests/test_treesolve_model.py computes and prints both --
                   and 100 x those figures exceed 1e-12: their limits are 1.5e-12 and 1.9e-12 (treesolve_model.LATTICE_OMEGA_LIMIT).
  forward error    |X - X_ref| / max |X_ref| per column against a CPU solve (np.linalg.solve; splu for M3500), limit SIG_RTOL = 1e-9,
                   the project's; two CPU references disagree by 1.2e-11 on M3500 (condition 7e8), 5e-12 on random3 and 2.2e-12 on the
                   700-pose graph.  Used on the non-lattice graphs only.
"""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets, harness
from tests.support.consumer_graphs import three_components, two_components
from tests.support.kernel_paths import KERNEL_PATHS
from tests.support.marginal_cases import case_arrays
from tests.support.selinv_model import sparse_system, system_blocks
from tests.support.sigma_compare import SIG_RTOL, Recorder, demo_checkpoints, dense as _dense
from tests.support.treesolve_model import LATTICE_OMEGA_LIMIT, OMEGA_LIMIT, backward_error, relative_covariances, rhs_columns
import tests.test_gpu_parity as T

pytestmark = pytest.mark.gpu
GATE_RTOL = 1e-9         # relative covariances against the numpy model and the gate (tests/test_gpu_gating.py)
# tests/test_gpu_consumer_paths.py's extra option sets, and those whose outputs are bitwise the default run's
EXTRA_PATHS = [dict(pool_guard=64), dict(pool_guard=64, small_lds_kb=0), dict(xcd_place=0), dict(amalg=1), dict(pool_poison=1)]
BITWISE = [dict(pool_guard=64), dict(xcd_place=0), dict(pool_poison=1)]
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _solved(lib, arr, steps=1):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    for _ in range(steps):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
    return g, p


def _system(g, p, lam_nodes=None):
    """the system the last step factorised, as a sparse matrix in node order"""
    states, fa, fb, z, W = g.arrays()
    Aii, Aab = system_blocks(g.l_points(), fa, fb, z, W, p.c.tikhanov, lam_nodes)
    return sparse_system(Aii, Aab, fa, fb).tocsc()


def _omega(g, p, B, X, limit=OMEGA_LIMIT, lam_nodes=None, what=""):
    """B, X: [nrhs, 3N] as the entry point takes them"""
    w = backward_error(_system(g, p, lam_nodes), X.T, B.T).max()
    print(f"[treesolve] {what}: omega {w:.3e} (limit {limit:.1e})")
    assert w < limit, (what, w)
    return w


def _rhs(N, nrhs, seed):
    return np.ascontiguousarray(rhs_columns(N, nrhs, seed).T)


# ---- 1. FULL against the CPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tutorial", "random0", "random1", "random2", "random3", "m3500"])
def test_full_solve_against_the_cpu(lib, name):
    arr = case_arrays(lib, name)
    g, p = _solved(lib, arr)
    N = len(arr[0])
    A = _system(g, p)
    if name == "m3500":
        import scipy.sparse.linalg as sla
        ref_solve = sla.splu(A).solve
    else:
        Ad = A.toarray()
        ref_solve = lambda b: np.linalg.solve(Ad, b)
    for nrhs in (1, 3, 16, 17, 33):
        B = _rhs(N, nrhs, 100 + nrhs)
        X = g.solve(p, B)
        assert X.shape == B.shape and np.isfinite(X).all()
        w = backward_error(A, X.T, B.T)
        ref = ref_solve(B.T)
        scale = np.abs(ref).max(axis=0)
        fe = np.where(scale > 0, np.abs(X.T - ref).max(axis=0) / np.where(scale > 0, scale, 1.0), np.abs(X.T).max(axis=0))
        print(f"[treesolve] {name} nrhs {nrhs}: omega {w.max():.3e}, forward error {fe.max():.3e}")
        assert w.max() < OMEGA_LIMIT, (name, nrhs, w.max())
        assert fe.max() < SIG_RTOL, (name, nrhs, fe.max())
        if nrhs > 2:
            assert np.all(X[2] == 0.0)                           # the zero column
    x1 = g.solve(p, B[0])                                        # a single vector of shape [3N]
    assert x1.shape == (3 * N,) and x1.tobytes() == X[0].tobytes()
    p.destroy(); g.destroy()


# ---- 2. front shapes and factor layouts --------------------------------------------------------------------------------------
ARR700 = datasets.random_pose_graph(700, 600, 21)


def _solve700(lib, opts):
    B = _rhs(len(ARR700[0]), 17, 21)
    with lib.options(**opts):
        g, p = _solved(lib, ARR700, 2)
        X = g.solve(p, B)
        _omega(g, p, B, X, what=f"random 700/600/21 {_ids(opts)}")
        lib.clear_error()
        g.cholesky(p)                                            # (pool_guard: the bands are checked after a synchronised step)
        assert lib.last_error()[0] == 0 and p.stats()["not_spd"] == 0
        p.destroy(); g.destroy()
    return X


@pytest.fixture(scope="module")
def default700(lib):
    return _solve700(lib, {})


@pytest.mark.parametrize("opts", KERNEL_PATHS + EXTRA_PATHS, ids=_ids)
def test_solve_behind_every_kernel_path(lib, default700, opts):
    X = _solve700(lib, opts)
    if opts in BITWISE:
        assert X.tobytes() == default700.tobytes(), opts


def _shape_cases():
    return [("random_3000", lambda lib: datasets.random_pose_graph(3000, 1800, 102), 17, OMEGA_LIMIT),
            ("star_3000", lambda lib: T._star(3000, 1), 17, OMEGA_LIMIT), ("star_70", lambda lib: T._star(70, 2), 17, OMEGA_LIMIT),
            ("chain_4000", lambda lib: T._chain(4000, 3), 17, OMEGA_LIMIT),
            ("two_components", lambda lib: two_components()[0], 17, OMEGA_LIMIT), ("three_components", lambda lib: three_components()[0], 17, OMEGA_LIMIT),
            ("lattice_60", lambda lib: lib.lattice_arrays(60), 17, LATTICE_OMEGA_LIMIT[60]),
            ("lattice_316", lambda lib: lib.lattice_arrays(316), 3, LATTICE_OMEGA_LIMIT[316])]


@pytest.mark.parametrize("name,make,nrhs,limit", _shape_cases(), ids=[c[0] for c in _shape_cases()])
def test_front_shapes(lib, name, make, nrhs, limit):
    """a root front of s = 1 935 = 120 tiles + 15, a front with 3 000 children, a deep thin tree, several roots (one front with s = 3
    and u = 0), the lattices"""
    arr = make(lib)
    N = len(arr[0])
    g, p = _solved(lib, arr)
    if name == "random_3000":
        assert p.stats()["max_front_rows"] > 1900
    seed = 60 if name == "lattice_60" else 316 if name == "lattice_316" else 7
    B = _rhs(N, nrhs, seed)
    X = g.solve(p, B)
    _omega(g, p, B, X, limit, what=name)
    assert np.all(X[2] == 0.0)
    p.destroy(); g.destroy()


# ---- 3. modes ----------------------------------------------------------------------------------------------------------------
def test_modes(lib):
    arr = case_arrays(lib, "random1")
    g, p = _solved(lib, arr)
    N = len(arr[0])
    Sig, scale = _dense(g, p)
    I = np.eye(3 * N)
    Fw = g.solve(p, I, "forward").T                              # columns: L^-1 e_j (permuted back)
    Bw = g.solve(p, I, "backward").T
    rs = np.repeat(scale, 3)[:, None]
    assert (np.abs(Fw.T @ Fw - Sig) / rs).max() < SIG_RTOL
    assert (np.abs(Bw @ Bw.T - Sig) / rs).max() < SIG_RTOL
    B = _rhs(N, 33, 3)
    full = g.solve(p, B)
    assert g.solve(p, g.solve(p, B, "forward"), "backward").tobytes() == full.tobytes()
    with lib.options(solve_chunk_cols=16):
        for mode in ("full", "forward", "backward"):
            chunked = g.solve(p, B, mode)
            with lib.options(solve_chunk_cols=0):
                assert g.solve(p, B, mode).tobytes() == chunked.tobytes(), mode
    X = B.copy()                                                 # in place
    assert lib.dll.aprilsam_amd_solve(g.ptr, p.ptr, 0, 33, X.ctypes.data_as(_dp), X.ctypes.data_as(_dp)) == 0
    assert X.tobytes() == full.tobytes()
    p.destroy(); g.destroy()


# ---- 4. cross ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random2", "m3500"])
def test_cross_covariances(lib, name):
    from tests.support.mf_emulator import PlanView
    arr = case_arrays(lib, name)
    g, p = _solved(lib, arr)
    N = len(arr[0])
    Sig, scale = _dense(g, p)
    P = PlanView(lib, N, arr[1], arr[2], xy=arr[0][:, :2])
    rng = np.random.default_rng(4)
    sub = rng.integers(0, N, 40).astype(np.int32)
    diag = g.marginals(p)
    for anchor in (0, N // 2, N - 1, int(P.perm[-1])):
        Cx = g.marginals_cross(p, anchor)
        ref = Sig[:, 3 * anchor:3 * anchor + 3].reshape(N, 3, 3)
        err = np.abs(Cx - ref).reshape(N, 9).max(axis=1) / np.maximum(scale, scale[anchor])
        assert err.max() < SIG_RTOL, (anchor, err.max())
        Cs = g.marginals_cross(p, anchor, sub)
        assert Cs.tobytes() == Cx[sub].tobytes()
        J = g.marginals_joint_any(p, sub, np.full(len(sub), anchor, np.int32))
        e2 = np.abs(Cs - J[:, :3, 3:]).reshape(len(sub), 9).max(axis=1) / np.maximum(scale[sub], scale[anchor])
        assert e2.max() < SIG_RTOL, (anchor, e2.max())
        assert np.abs(Cx[anchor] - diag[anchor]).max() < SIG_RTOL * scale[anchor]
    p.destroy(); g.destroy()


def test_cross_covariance_across_components_is_zero(lib):
    arr, comp = three_components()
    g, p = _solved(lib, arr, 2)
    for anchor in (5, 450, int(np.nonzero(comp == 2)[0][0])):
        Cx = g.marginals_cross(p, anchor)
        other = comp != comp[anchor]
        assert np.all(Cx[other] == 0.0) and np.abs(Cx[~other]).max() > 0
    p.destroy(); g.destroy()


# ---- 5. relative covariances ----------------------------------------------------------------------------------------------------
def test_relative_covariances(lib):
    arr = case_arrays(lib, "random2")
    g, p = _solved(lib, arr, 2)                                  # states != l_points
    N = len(arr[0])
    assert not np.array_equal(g.states(), g.l_points())
    Sig, _ = _dense(g, p)
    runs = lib.dll.aprilsam_amd_debug_selinv_runs
    r0 = runs(p.ptr)
    for anchor in (N - 1, 0, N // 2):
        R = g.relative_covariances(p, anchor)
        nodes = np.arange(N)
        Sii = np.stack([Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in nodes])
        Sia = Sig[:, 3 * anchor:3 * anchor + 3].reshape(N, 3, 3)
        model = relative_covariances(g.states(), anchor, nodes, Sig[3 * anchor:3 * anchor + 3, 3 * anchor:3 * anchor + 3], Sii, Sia)
        others = nodes[nodes != anchor].astype(np.int32)
        a = np.full(len(others), anchor, np.int32)
        _, S = g.gate_xyt(p, a, others, np.zeros((len(others), 3)), np.tile(np.eye(3).reshape(9), (len(others), 1)))
        big = np.abs(model[others]).max(axis=(1, 2))
        assert (np.abs(R[others] - model[others]).max(axis=(1, 2)) / big).max() < GATE_RTOL
        assert (np.abs(R[others] - (S - np.eye(3))).max(axis=(1, 2)) / big).max() < GATE_RTOL
        assert np.all(R[anchor] == 0.0)
        sub = np.array([anchor, 1, 7, anchor, N - 2], np.int32)
        assert g.relative_covariances(p, anchor, sub).tobytes() == R[sub].tobytes()
    assert runs(p.ptr) == r0 + 1                                 # the first call ran the selected inversion, the later ones did not
    p.destroy(); g.destroy()


# ---- 6. incremental structure ---------------------------------------------------------------------------------------------------
def test_incremental_demo_checkpoints_and_non_interference(lib):
    """first 300 steps of the M3500 incremental demo (batch, re-planned, low-rank-updated and fast-path checkpoints): FULL with three
    columns, then the cross blocks of the newest pose against joint_any; the demo's results bitwise those of a run without the calls"""
    arr = datasets.m3500_arrays()
    plain = harness.run_demo(lib, arr, max_poses=300, record_states_every=50)
    rec = Recorder(lib)

    def check(g, p, k, lam_nodes):
        N = g.n_nodes
        B = _rhs(N, 3, k)
        X = g.solve(p, B)
        _omega(g, p, B, X, lam_nodes=lam_nodes, what=f"demo step {k} ({N} poses)")
        nodes = np.unique(np.r_[np.arange(min(N, 10)), np.random.default_rng(k).integers(0, N, 20), N - 1]).astype(np.int32)
        Cx = g.marginals_cross(p, N - 1, nodes)
        J = g.marginals_joint_any(p, nodes, np.full(len(nodes), N - 1, np.int32))
        scale = np.abs(J).max(axis=(1, 2))
        assert (np.abs(Cx - J[:, :3, 3:]).max(axis=(1, 2)) / scale).max() < SIG_RTOL
    on_step, seen = demo_checkpoints(rec, arr, check)
    res = harness.run_demo(rec, arr, max_poses=300, record_states_every=50, on_step=on_step)
    assert seen["batch"] >= 1 and seen["replanned"] >= 1 and seen["updated"] >= 1 and seen["fast"] >= 1, seen
    print(f"[treesolve] demo checkpoints: {seen}")
    assert res["chi2"].tobytes() == plain["chi2"].tobytes()
    assert res["final_states"].tobytes() == plain["final_states"].tobytes()
    for k in plain["snaps"]:
        assert res["snaps"][k].tobytes() == plain["snaps"][k].tobytes()


# ---- 7. state and refusals --------------------------------------------------------------------------------------------------------
def test_after_batch_resident(lib):
    arr = case_arrays(lib, "random1")
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    g.batch_resident(p, 3)
    N = len(arr[0])
    B = _rhs(N, 5, 1)
    _omega(g, p, B, g.solve(p, B), what="after batch_resident")
    Sig, scale = _dense(g, p)
    Cx = g.marginals_cross(p, 3)
    assert (np.abs(Cx - Sig[:, 9:12].reshape(N, 3, 3)).reshape(N, 9).max(axis=1) / np.maximum(scale, scale[3])).max() < SIG_RTOL
    R = g.relative_covariances(p, 3)
    assert np.isfinite(R).all() and np.all(R[3] == 0.0) and np.abs(R).max() > 0
    p.destroy(); g.destroy()


def _raw(lib, g, p, what, *args):
    """the raw entry point on sentinel-filled output: (return code, output untouched, last_error code)"""
    d = lib.dll
    lib.clear_error()
    if what == "solve":
        mode, nrhs, B = args
        X = np.full((max(nrhs, 1), B.shape[-1]) if B is not None else 8, -7.0)
        rc = d.aprilsam_amd_solve(g.ptr if g else None, p.ptr if p else None, mode, nrhs, B.ctypes.data_as(_dp) if B is not None else None, X.ctypes.data_as(_dp))
        out = X
    else:
        anchor, nodes = args
        n = 0 if nodes is None else len(nodes)
        out = np.full((g.n_nodes if nodes is None else n, 9), -7.0)
        idx = None if nodes is None else np.ascontiguousarray(nodes, np.int32)
        fn = d.aprilsam_amd_marginals_cross if what == "cross" else d.aprilsam_amd_relative_covariances
        rc = fn(g.ptr, p.ptr if p else None, anchor, n, idx.ctypes.data_as(_ip) if idx is not None else None, out.ctypes.data_as(_dp))
    return rc, bool(np.all(out == -7.0)), lib.last_error()[0]


def test_refusals_leave_everything_untouched(lib):
    arr = case_arrays(lib, "lattice60")
    N = len(arr[0])
    ref_g, ref_p = _solved(lib, arr, 2)
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    B = _rhs(N, 2, 1)

    def refused(code, what, *args, gg=None, pp=None):
        rc, untouched, err = _raw(lib, gg or g, pp or p, what, *args)
        assert (rc, untouched, err) == (code, True, code), (what, args[:2], rc, untouched, err)
    # -1: a fresh param
    refused(-1, "solve", 0, 2, B); refused(-1, "cross", 0, None); refused(-1, "relative", 0, None)
    g.cholesky(p)
    r0 = lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)
    # -13
    refused(-13, "solve", 3, 2, B); refused(-13, "solve", -1, 2, B); refused(-13, "solve", 0, 0, B); refused(-13, "solve", 0, 2, None)
    assert lib.dll.aprilsam_amd_solve(g.ptr, p.ptr, 0, 2, B.ctypes.data_as(_dp), None) == -13
    assert lib.dll.aprilsam_amd_solve(g.ptr, None, 0, 2, B.ctypes.data_as(_dp), B.ctypes.data_as(_dp)) == -13
    for what in ("cross", "relative"):
        refused(-13, what, N, None); refused(-13, what, -1, None); refused(-13, what, 0, [1, N]); refused(-13, what, 0, [-1])
        fn = lib.dll.aprilsam_amd_marginals_cross if what == "cross" else lib.dll.aprilsam_amd_relative_covariances
        assert fn(g.ptr, p.ptr, 0, 0, None, None) == -13
    # -11: the work buffer under mem_cap_mb
    with lib.options(mem_cap_mb=1):
        B64 = _rhs(N, 64, 2)
        lib.clear_error()
        X = np.full_like(B64, -7.0)
        assert lib.dll.aprilsam_amd_solve(g.ptr, p.ptr, 0, 64, B64.ctypes.data_as(_dp), X.ctypes.data_as(_dp)) == -11
        assert np.all(X == -7.0) and lib.last_error()[0] == -11
    # -12: a sharded param, an asymmetric W
    d = lib.dll
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    d.aprilsam_amd_shard_end.argtypes = [C.c_void_p]
    g3, p3 = _solved(lib, arr)
    assert d.aprilsam_amd_shard_begin(C.cast(g3.ptr, C.c_void_p), C.cast(p3.ptr, C.c_void_p), 0, 1) == 0
    refused(-12, "solve", 0, 2, B, gg=g3, pp=p3); refused(-12, "cross", 0, None, gg=g3, pp=p3); refused(-12, "relative", 0, None, gg=g3, pp=p3)
    d.aprilsam_amd_shard_end(C.cast(p3.ptr, C.c_void_p))
    from tests.support.asym_scenarios import batch_graph
    ga, pa = _solved(lib, batch_graph())
    Ba = np.ones((1, 3 * ga.n_nodes))
    refused(-12, "solve", 0, 1, Ba, gg=ga, pp=pa); refused(-12, "cross", 0, None, gg=ga, pp=pa); refused(-12, "relative", 0, None, gg=ga, pp=pa)
    # -1 after optimize_lm: the factor is dropped
    gl, pl = _solved(lib, case_arrays(lib, "random1"))
    gl.optimize_lm(pl, max_iters=3)
    Bl = np.ones((1, 3 * gl.n_nodes))
    refused(-1, "solve", 0, 1, Bl, gg=gl, pp=pl); refused(-1, "cross", 0, None, gg=gl, pp=pl); refused(-1, "relative", 0, None, gg=gl, pp=pl)
    # -1 while a resident run is in progress; after resident_end the calls work again
    gr, pr = _solved(lib, case_arrays(lib, "random1"))
    Nr = gr.n_nodes
    assert d.aprilsam_amd_factorised_nodes(pr.ptr) == Nr
    assert d.aprilsam_amd_resident_begin(gr.ptr, pr.ptr) == 0
    assert d.aprilsam_amd_resident_steps(gr.ptr, pr.ptr, 1, 0) == 0
    refused(-1, "solve", 0, 1, Bl, gg=gr, pp=pr); refused(-1, "cross", 0, None, gg=gr, pp=pr); refused(-1, "relative", 0, None, gg=gr, pp=pr)
    assert d.aprilsam_amd_factorised_nodes(pr.ptr) == -1
    assert d.aprilsam_amd_resident_sync(gr.ptr, pr.ptr) == 0 and d.aprilsam_amd_resident_end(gr.ptr, pr.ptr) == 0
    _omega(gr, pr, Bl, gr.solve(pr, Bl), what="after resident_end")
    assert gr.marginals_cross(pr, 0).shape == (Nr, 3, 3) and gr.relative_covariances(pr, 0).shape == (Nr, 3, 3)
    # -13 for relative_covariances: inside the factorised system but beyond the nodes of the graph that is passed
    gs = lib.new_graph(); gs.build_from_arrays(*case_arrays(lib, "random0"))
    assert gs.n_nodes < 20 < N
    refused(-13, "relative", 20, [1], gg=gs); refused(-13, "relative", 0, [20], gg=gs); refused(-13, "relative", 0, None, gg=gs)
    # the Python wrapper refuses a right-hand side of the wrong length before the library reads it
    with pytest.raises(ValueError):
        g.solve(p, np.ones(3 * N - 3))
    with pytest.raises(ValueError):
        g.solve(p, np.ones((2, 3 * N + 3)))
    # nothing moved: no selected inversion ran, the next calls and the next solver step give the bits of a run without the refusals
    assert lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr) == r0
    one_g, one_p = _solved(lib, arr)
    assert g.solve(p, B).tobytes() == one_g.solve(one_p, B).tobytes()
    assert g.marginals(p).tobytes() == one_g.marginals(one_p).tobytes()
    g.cholesky(p)
    assert g.states().tobytes() == ref_g.states().tobytes()
    assert g.solve(p, B).tobytes() == ref_g.solve(ref_p, B).tobytes()
    for x in (p, g, ref_p, ref_g, p3, g3, one_p, one_g, pa, ga, pl, gl, pr, gr, gs):
        x.destroy()


def test_batch_steps_are_bitwise_unaffected_and_calls_repeat(lib):
    arr = datasets.random_pose_graph(400, 350, 2)
    N = len(arr[0])
    B = _rhs(N, 5, 8)
    runs = []
    for with_s in (False, True):
        g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        snaps = []
        for k in range(20):
            g.cholesky(p)
            if with_s:
                x1 = g.solve(p, B, ("full", "forward", "backward")[k % 3]); x2 = g.solve(p, B, ("full", "forward", "backward")[k % 3])
                c1 = g.marginals_cross(p, k); c2 = g.marginals_cross(p, k)
                r1 = g.relative_covariances(p, k, [0, k, N - 1]); r2 = g.relative_covariances(p, k, [0, k, N - 1])
                assert x1.tobytes() == x2.tobytes() and c1.tobytes() == c2.tobytes() and r1.tobytes() == r2.tobytes()
            snaps.append(np.concatenate([g.states(), g.deltas(), g.l_points()]).tobytes())
        runs.append(snaps)
        p.destroy(); g.destroy()
    assert runs[0] == runs[1]


def test_params_on_two_slots(lib):
    arr = case_arrays(lib, "lattice24")
    N = len(arr[0])
    B = _rhs(N, 5, 6)
    out = []
    for slots in ((0, 0), (0, 1)):
        gs, ps = [], []
        for s in slots:
            g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
            assert lib.dll.aprilsam_amd_param_set_device(p.ptr, s) == 0
            g.cholesky(p); gs.append(g); ps.append(p)
        x = [g.solve(p, B) for g, p in zip(gs, ps)]
        cx = [g.marginals_cross(p, 7) for g, p in zip(gs, ps)]
        rl = [g.relative_covariances(p, 7) for g, p in zip(gs, ps)]
        for g, p in zip(gs, ps):
            g.cholesky(p)
        out.append([v.tobytes() for v in x + cx + rl] + [g.states().tobytes() for g in gs])
        for v in gs + ps:
            v.destroy()
    assert out[0][0] == out[0][1] == out[1][0] == out[1][1]
    assert out[0][2] == out[0][3] == out[1][2] == out[1][3] and out[0][4] == out[0][5] == out[1][4] == out[1][5]
    assert out[0][6:] == out[1][6:]
