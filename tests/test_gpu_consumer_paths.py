"""The consumers of the retained factor -- selected inversion (aprilsam_amd_marginals, _marginals_joint: aprilsam_amd/csrc/selinv.hip.h)
and path solves (aprilsam_amd_marginals_joint_any, aprilsam_amd_gate_xyt: pathsolve.hip.h) -- behind every kernel path of the batch
step.  They read L_SS and L_US straight from the front pool through tables rebuilt from the plan, and DESIGN.md section 11 says that
they do not depend on which path factorised a front: here every option set of tests/support/kernel_paths.py (which kernel wrote a
front), the options that move offsets and change the tree (pool_guard, leaf_nodes, pin_last, amalg, xcd_place), the wide root front
ending in a partial outer block, the lattice, a graph with several roots and the star and chain trees run through them.

Tolerances are the project's own (tests/support/sigma_compare.py, tests/test_gpu_gating.py, tests/test_gpu_marginals.py):
SIG_RTOL = 1e-9 of the block row's largest entry against the dense inverse, GATE_RTOL = 1e-9 against the numpy gating model,
SPLU_RTOL = 1e-8 against splu solves, IDENT_RTOL = 1e-9 for the identity residual.  Two CPU references of Sigma -- the dense inverse
against splu with COLAMD and with MMD -- disagree, by the same scale, by at most 3.1e-12 (random 700 / 600 / 21), 2.9e-12 (random
3000 / 1800 / 102) and 8.4e-13 (the two-component graph): 1e-9 keeps the 300 x margin it has on the graphs it was calibrated on."""
import ctypes as C

import numpy as np
import pytest

from aprilsam_amd import datasets
from tests.support.consumer_graphs import three_components, two_components
from tests.support.gate_model import gate, gate_inputs
from tests.support.kernel_paths import KERNEL_PATHS
from tests.support.marginal_cases import factor_pairs
from tests.support.marginal_identity import identity_residual
from tests.support.selinv_model import dense_system, sparse_system, system_blocks
from tests.support.sigma_compare import SIG_RTOL, check_any, check_blocks, random_pairs, ref_joint, row_scale
import tests.test_gpu_parity as T

pytestmark = pytest.mark.gpu
GATE_RTOL = 1e-9         # d2 and S against the numpy model (tests/test_gpu_gating.py)
SPLU_RTOL = 1e-8         # against splu solves (tests/test_gpu_marginals.py)
IDENT_RTOL = 1e-9        # identity residual (tests/test_gpu_marginals.py)

# pool_guard moves every front's offset; xcd_place = 0 lists the fronts of the multi-level launches level by level; amalg merges
# separator fronts; pool_poison fills what a step hands over with NaN first
EXTRA_PATHS = [dict(pool_guard=64), dict(pool_guard=64, small_lds_kb=0), dict(xcd_place=0), dict(amalg=1), dict(pool_poison=1)]
# the same kernels on the same numbers as the default options (guard bands only move offsets, placement only reorders work lists,
# poison is overwritten before it is read): the outputs bitwise those of the default run
BITWISE = [dict(pool_guard=64), dict(xcd_place=0), dict(pool_poison=1)]
# What shows that an option set took effect: "fronts on the multi-workgroup path" of aprilsam_amd_level_profile under small_lds_kb=0,
# stats.n_fronts against the default under leaf_nodes / pin_last / amalg.  The library exposes nothing that tells the remaining sets
# apart (LDS budgets above 0, panel_mode, workgroup sizes, tp_fronts, schur_first, the syrk_* tilings, blk_backsolve, wave_backsolve,
# use_graph, persist*, linearize_staged_min, trust_factor_cache, xcd_place, pool_poison, pool_guard; device_timing shows in
# stats.ms_dev_factor): they run all the same, as they do in tests/test_gpu_parity.py.
CHANGES_THE_TREE = ("leaf_nodes", "pin_last", "amalg")


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _solved(lib, arr, steps):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    for _ in range(steps):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
    return g, p


def _dense_at(lp, arr, lam=1e-4):
    """(Sigma, row scales) of the system linearised at lp"""
    states, fa, fb, z, W = arr
    Aii, Aab = system_blocks(lp, fa, fb, z, W, lam)
    Sig = np.linalg.inv(dense_system(Aii, Aab, fa, fb))
    return Sig, row_scale(Sig)


def _multi_workgroup_fronts(lib, arr):
    """fronts on the multi-workgroup path under the options in force (aprilsam_amd_level_profile after one instrumented resident pass
    on a param of its own)"""
    d = lib.dll
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 1, 1) == 0
    assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
    assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    lv = (C.c_double * (6 * 64))()
    d.aprilsam_amd_level_profile.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    nl = d.aprilsam_amd_level_profile(C.cast(p.ptr, C.c_void_p), lv, 64)
    assert nl > 0
    n = sum(int(lv[6 * l + 3]) for l in range(min(nl, 64)))
    p.destroy(); g.destroy()
    return n


def _consumers(lib, arr, opts, steps, pairs, n_gate=50, ref=None):
    """`steps` batch steps and every consumer inside lib.options(**opts), all of it checked against the dense inverse of the system
    the last step factorised (ref: that inverse when the caller has it).  Returns the outputs and the stats"""
    states, fa, fb, z, W = arr
    pa, pb = factor_pairs(fa, fb)
    a, b = pairs
    ga, gb, gz, gW = gate_inputs(arr, n_gate, 5)
    with lib.options(**opts):
        g, p = _solved(lib, arr, steps)
        out = dict(diag=g.marginals(p))
        out["joint"] = g.marginals_joint(p, pa, pb)
        out["any"] = g.marginals_joint_any(p, a, b)
        out["d2"], out["S"] = g.gate_xyt(p, ga, gb, gz, gW)
        out["gate_any"] = g.marginals_joint_any(p, ga, gb)
        stats = p.stats()
        if opts.get("small_lds_kb", 156) == 0:
            assert _multi_workgroup_fronts(lib, arr) > 0, opts
        x, lp = g.states(), g.l_points()
        p.destroy(); g.destroy()
    for k, v in out.items():
        assert not np.isnan(v).any(), (opts, k)
    if ref is None:
        ref = _dense_at(lp, arr)
    else:                                                        # (a reference computed before: for the system at the graph's own states)
        assert steps == 1 and np.array_equal(lp, states)
    worst = dict(blocks=check_blocks(ref, fa, fb, out["diag"], out["joint"]), any=check_any(ref, a, b, out["any"]),
                 gate_any=check_any(ref, ga, gb, out["gate_any"]))
    # the gate as tests/test_gpu_gating.test_gate_matches_the_model checks it: the model on the library's own joint blocks (which the
    # lines above hold to the dense inverse) at GATE_RTOL, and on the dense inverse's blocks at 1e-7 of every d2
    md2, mS = gate(x, ga, gb, gz, gW, out["gate_any"])
    d2, S = out["d2"], out["S"]
    assert np.abs(d2 - md2).max() < GATE_RTOL * np.abs(md2).max() and (np.abs(d2 - md2) <= GATE_RTOL * np.abs(md2) + 1e-300).all(), opts
    assert np.abs(S - mS).max() < GATE_RTOL * np.abs(mS).max(), opts
    md2b, _ = gate(x, ga, gb, gz, gW, ref_joint(ref[0], ga, gb))
    assert (np.abs(d2 - md2b) <= 1e-7 * np.abs(md2b)).all(), opts
    print(f"[consumers] {_ids(opts)}: fronts {stats['n_fronts']} levels {stats['n_levels']} worst {worst}")
    return out, stats


def _same_bits(out, base, what):
    for k, v in base.items():
        assert v.tobytes() == out[k].tobytes(), (what, k, float(np.max(np.abs(v - out[k]))))


# ---- 1. the matrix's own graph under every kernel path ------------------------------------------------------------------------
ARR700 = datasets.random_pose_graph(700, 600, 21)


def _pairs700():
    a, b = random_pairs(len(ARR700[0]), 1)                       # both orders and a == b
    fa, fb = factor_pairs(ARR700[1], ARR700[2])
    return np.r_[a, fa].astype(np.int32), np.r_[b, fb].astype(np.int32)


@pytest.fixture(scope="module")
def default700(lib):
    return _consumers(lib, ARR700, {}, 2, _pairs700())


@pytest.fixture(scope="module")
def big_path700(lib):
    return _consumers(lib, ARR700, dict(small_lds_kb=0), 2, _pairs700())


@pytest.mark.parametrize("opts", KERNEL_PATHS + EXTRA_PATHS, ids=_ids)
def test_consumers_behind_every_kernel_path(lib, default700, big_path700, opts):
    """two batch steps, then marginals of all poses, marginals_joint of every factor pair, joint_any of random pairs (both orders,
    a == b) and of the factor pairs, and 50 gated candidates -- all inside the option scope"""
    out, stats = _consumers(lib, ARR700, opts, 2, _pairs700())
    base, base_stats = default700
    if any(k in opts for k in CHANGES_THE_TREE):
        assert stats["n_fronts"] != base_stats["n_fronts"], (opts, stats["n_fronts"])
    if "device_timing" in opts:
        assert stats["ms_dev_factor"] > 0
    if opts in BITWISE:
        _same_bits(out, base, opts)
    if opts == dict(pool_guard=64, small_lds_kb=0):              # (guard bands on the multi-workgroup path: against that path's own run)
        _same_bits(out, big_path700[0], opts)


# ---- the root front of 645 poses: 15 outer blocks and a partial one, the last array of the pool -------------------------------
ARR3000 = datasets.random_pose_graph(3000, 1800, 102)


@pytest.fixture(scope="module")
def dense3000():
    """one batch step factorises the system at the graph's own states, whatever the options: one inverse (9 000 unknowns) serves
    every option set"""
    return _dense_at(ARR3000[0], ARR3000)


@pytest.mark.parametrize("opts", [{}, dict(small_lds_kb=0), dict(blk_backsolve=0, small_lds_kb=0), dict(syrk_pair_tiles=1, syrk_group=3, small_lds_kb=0)],
                         ids=_ids)
def test_wide_root_front_ending_in_a_partial_outer_block(lib, dense3000, opts):
    rng = np.random.default_rng(102)
    N = len(ARR3000[0])
    pairs = (rng.integers(0, N, 200).astype(np.int32), rng.integers(0, N, 200).astype(np.int32))
    out, stats = _consumers(lib, ARR3000, opts, 1, pairs, ref=dense3000)
    assert stats["max_front_rows"] > 1900


# ---- the lattice ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice60(lib):
    arr = lib.lattice_arrays(60)
    return arr, _dense_at(arr[0], arr)


@pytest.fixture(scope="module")
def default_lattice60(lib, lattice60):
    arr, ref = lattice60
    return _consumers(lib, arr, {}, 1, random_pairs(len(arr[0]), 3), ref=ref)


@pytest.mark.parametrize("opts", [dict(small_lds_kb=0), dict(panel_mode=0, small_lds_kb=64), dict(leaf_nodes=4), dict(pin_last=12), dict(pool_guard=64)],
                         ids=_ids)
def test_lattice_behind_other_paths(lib, lattice60, default_lattice60, opts):
    arr, ref = lattice60
    out, stats = _consumers(lib, arr, opts, 1, random_pairs(len(arr[0]), 3), ref=ref)
    if any(k in opts for k in CHANGES_THE_TREE):
        assert stats["n_fronts"] != default_lattice60[1]["n_fronts"], (opts, stats["n_fronts"])
    if opts in BITWISE:
        _same_bits(out, default_lattice60[0], opts)


# ---- several roots ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, dict(small_lds_kb=0)], ids=_ids)
@pytest.mark.parametrize("make", [two_components, three_components], ids=["two", "three"])
def test_disconnected_graph(lib, make, opts):
    """random 400 / 350 / 2 and random 80 / 60 / 1 side by side, each with its prior (and a third component of one pose with only a
    prior): several roots.  Within a component everything as on a connected graph; across components marginals_joint has no block
    (all NaN, counted), joint_any has the two marginals and a zero cross block (PsPair::nc == 0), the gate follows the model"""
    arr, comp = make()
    states, fa, fb, z, W = arr
    N = len(states)
    rng = np.random.default_rng(7)
    a = rng.integers(0, N, 300).astype(np.int32); b = rng.integers(0, N, 300).astype(np.int32)
    lone = np.nonzero(comp == 2)[0]
    if len(lone):                                                # the lone pose against both other components, both orders, and itself
        a = np.r_[a, lone[0], 5, lone[0], 450, lone[0]].astype(np.int32); b = np.r_[b, 5, lone[0], 450, lone[0], lone[0]].astype(np.int32)
    cross = comp[a] != comp[b]
    assert cross.sum() > 50 and (~cross).sum() > 50
    out, stats = _consumers(lib, arr, opts, 2, (a, b))           # (dense inverse: diagonal blocks, factor pairs, joint_any, the gate)
    with lib.options(**opts):
        g, p = _solved(lib, arr, 2)
        J = g.marginals_joint_any(p, a, b)
        d = g.marginals(p)
        on = np.empty((len(a), 6, 6))
        rc = lib.dll.aprilsam_amd_marginals_joint(g.ptr, p.ptr, len(a), a.ctypes.data_as(C.POINTER(C.c_int)), b.ctypes.data_as(C.POINTER(C.c_int)),
                                                  on.ctypes.data_as(C.POINTER(C.c_double)))
        ga, gb, gz, gW = gate_inputs(arr, 200, 9)
        d2, S = g.gate_xyt(p, ga, gb, gz, gW)
        Jg = g.marginals_joint_any(p, ga, gb)
        x = g.states()
        p.destroy(); g.destroy()
    assert J.tobytes() == out["any"].tobytes()
    # marginals_joint: no pair of two components lies on the pattern of L
    off = np.isnan(on).all(axis=(1, 2))
    assert rc == int(off.sum()) and off[cross].all() and not np.isnan(on[~off]).any()
    # joint_any across components: finite, its diagonal blocks the marginals, its cross block zero
    Jc = J[cross]
    assert np.isfinite(Jc).all()
    # (the path solves and the selected inversion reach Sigma_aa by different sums: equal to SIG_RTOL of the larger marginal's largest
    # entry -- a scale no larger than the block row's -- not bit for bit)
    scale = np.maximum(np.abs(d[a[cross]]).max(axis=(1, 2)), np.abs(d[b[cross]]).max(axis=(1, 2)))
    dd = np.maximum(np.abs(Jc[:, :3, :3] - d[a[cross]]).max(axis=(1, 2)), np.abs(Jc[:, 3:, 3:] - d[b[cross]]).max(axis=(1, 2))) / scale
    assert dd.max() < SIG_RTOL, dd.max()
    xb = np.abs(Jc[:, :3, 3:]).max(axis=(1, 2))
    print(f"[disconnected] {_ids(opts)}: diagonal blocks against marginals {dd.max():.2e}; largest cross block entry across components "
          f"{xb.max():.3e} (expected exactly 0.0)")
    assert (xb <= SIG_RTOL * scale).all() and (np.abs(Jc[:, 3:, :3]).max(axis=(1, 2)) <= SIG_RTOL * scale).all()
    # the gate across components
    gx = comp[ga] != comp[gb]
    assert gx.sum() > 20
    md2, mS = gate(x, ga, gb, gz, gW, Jg)
    assert (np.abs(d2 - md2) <= GATE_RTOL * np.abs(md2) + 1e-300).all() and np.abs(S - mS).max() < GATE_RTOL * np.abs(mS).max()
    assert np.abs(d2[gx] - md2[gx]).max() < GATE_RTOL * np.abs(md2[gx]).max()


# ---- star and chain trees -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,arr", [("star_3000", T._star(3000, 1)), ("star_70", T._star(70, 2)), ("chain_4000", T._chain(4000, 3))])
def test_degenerate_tree_shapes(lib, name, arr):
    """a root front with thousands of children and a deep, thin tree: the identity sum_j A_ij Sigma_ji = I over all poses, and 64 poses
    and 64 pairs -- half of them not joined by a factor -- against splu solves (marginals, marginals_joint, joint_any)"""
    import scipy.sparse.linalg as sla
    states, fa, fb, z, W = arr
    N = len(states)
    g, p = _solved(lib, arr, 1)
    Aii, Aab = system_blocks(g.l_points(), fa, fb, z, W, p.c.tikhanov)
    pa, pb = factor_pairs(fa, fb)
    diag = g.marginals(p)
    jf = np.zeros((len(fa), 6, 6)); jf[fb >= 0] = g.marginals_joint(p, pa, pb)
    res = identity_residual(Aii, Aab, fa, fb, diag, jf)
    assert res["rel_max"] < IDENT_RTOL, res["rel_max"]
    lu = sla.splu(sparse_system(Aii, Aab, fa, fb).tocsc())
    rng = np.random.default_rng(len(name))
    poses = rng.choice(N, 64, replace=False)
    k = rng.choice(len(pa), 32, replace=False)
    joined = set(zip(pa.tolist(), pb.tolist())) | set(zip(pb.tolist(), pa.tolist()))
    fa_, fb_ = [], []
    while len(fa_) < 32:                                         # 32 pairs no factor joins
        x, y = (int(v) for v in rng.integers(0, N, 2))
        if x != y and (x, y) not in joined:
            fa_.append(x); fb_.append(y)
    a = np.r_[pa[k], fa_].astype(np.int32); b = np.r_[pb[k], fb_].astype(np.int32)
    J = g.marginals_joint_any(p, a, b)
    on = g.marginals_joint(p, a[:32], b[:32])
    worst = 0.0
    for i, n in enumerate(poses):
        E = np.zeros((3 * N, 3)); E[3 * n:3 * n + 3] = np.eye(3)
        col = lu.solve(E)
        e = np.abs(diag[n] - col[3 * n:3 * n + 3]).max() / np.abs(col).max()
        worst = max(worst, e)
        assert e < SPLU_RTOL, (name, n, e)
    for i in range(len(a)):
        E = np.zeros((3 * N, 6)); E[3 * a[i]:3 * a[i] + 3, :3] = np.eye(3); E[3 * b[i]:3 * b[i] + 3, 3:] = np.eye(3)
        col = lu.solve(E)
        ref = np.vstack([col[3 * a[i]:3 * a[i] + 3], col[3 * b[i]:3 * b[i] + 3]])
        e = np.abs(J[i] - ref).max() / np.abs(col).max()
        worst = max(worst, e)
        assert e < SPLU_RTOL, (name, i, e)
        if i < 32:
            assert np.abs(on[i] - ref).max() < SPLU_RTOL * np.abs(col).max(), (name, i)
    print(f"[degenerate] {name}: identity {res['rel_max']:.2e}, worst against splu {worst:.2e}")
    p.destroy(); g.destroy()
