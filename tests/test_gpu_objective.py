"""The objective on the GPU: one evaluator under two conventions -- april_graph_chi2's (CHI2) and the least-squares
objective of LM, GNC and chordal (LM) -- and one reducer behind both.  Every family's term under each convention against the numpy models
the families' own tests use, the two conventions against each other, and the two-stage forms of the reducer (more than 65 536 terms) that
LM's sum and GNC's maximum take."""
import math

import numpy as np
import pytest

from tests.support import lm_model, maxmix_model, polar_model, robust_model
from tests.support import marginal_prior_model as mm
from tests.support.normal_eq import linearise
from tests.support.retained_contract import CLOSURES, LOOP, FamCtx

pytestmark = pytest.mark.gpu

# one evaluation of the objective against a numpy model: the relative bound of every family's own GPU test for the same quantity
# (tests/test_gpu_robust.py, test_gpu_lm.py, test_gpu_polar.py, test_gpu_gaussian.py and test_gpu_gnc.py all use 1e-12 for chi2 and F_initial)
TERM_RTOL = 1e-12
# a sum of 397 531 terms against the exactly rounded sum: tests/test_gpu_api_surface.py::test_chi2_of_a_large_graph_sums_in_two_stages_reproducibly
SUM_RTOL = 1e-13
REDUCE_SPLIT = 1 << 16           # kernels.hip.h: more terms than this are reduced in two stages


# ---- 1. all families in one graph -------------------------------------------------------------------------------------------------------
def _families_model(ctx, x):
    """(chi2, F) of the families scene at x: the sum of the numpy models' terms under each convention"""
    fam = ctx.fam
    plain = (np.array(ctx.fa), np.array(ctx.fb), np.array(ctx.z), np.array(ctx.W))
    rb, mx = fam["robust"], fam["mix"]
    rb_plain = (np.array([rb["a"]]), np.array([rb["b"]]), np.array([rb["z"]]), np.array([rb["W"]]))
    mixes = [(mx["a"], mx["b"], mx["zs"], mx["Ws"], mx["logw"])]
    polars = [tuple(p) for p in fam["polars"]]
    nodes, xbar, eta, Lam = fam["gauss"]
    _, _, c0 = mm.sqrt_form(eta, Lam, np.longdouble)                  # (as tests/support/gaussian_graphs.model_chi2)
    gauss = float(mm.gaussian_chi2(x, nodes, xbar, eta, Lam, c0, np.longdouble))
    chi2 = (polar_model.chi2(x, plain, polars) + robust_model.chi2(x, rb_plain, rb["kind"], rb["c"])
            + maxmix_model.chi2(x, polar_model.NO_PLAIN, mixes) + gauss)
    F = (polar_model.cost(x, plain, polars) + robust_model.cost(x, rb_plain, rb["kind"], rb["c"])
         + lm_model.cost(x, polar_model.NO_PLAIN, mixes) + gauss)
    return chi2, F


def _families_run(lib):
    ctx = FamCtx(lib)
    chi2 = ctx.g.chi2()
    F = ctx.g.optimize_lm(ctx.p, max_iters=1)["F_initial"]
    ctx.p.destroy(); ctx.g.destroy()
    return ctx, chi2, F


def test_every_family_under_both_conventions(lib):
    """plain xyt and a prior, a Cauchy closure, a two-component mixture, two range-bearing factors and a dense Gaussian factor in one graph:
    april_graph_chi2 and LM's F at the start against the models' terms; the same bits without graph capture"""
    ctx, chi2, F = _families_run(lib)
    want_chi2, want_F = _families_model(ctx, np.array(ctx.sc["start"], float))
    print("chi2", chi2, want_chi2, abs(chi2 - want_chi2) / want_chi2, "F", F, want_F, abs(F - want_F) / want_F)
    assert abs(chi2 - want_chi2) <= TERM_RTOL * want_chi2
    assert abs(F - want_F) <= TERM_RTOL * want_F
    with lib.options(use_graph=0):
        _, chi2_plain, F_plain = _families_run(lib)
    assert (chi2_plain, F_plain) == (chi2, F)


def test_chi2_inside_a_gnc_call_is_the_plain_one(lib):
    """the surrogate of the candidates is the LM convention's alone: chi2_final, taken while the candidates' table is still active, is
    what a fresh april_graph_chi2 returns"""
    ctx = FamCtx(lib)
    cand = np.array([LOOP + 0, LOOP + 1], np.int32)                  # factor 0 the prior, 1 .. 39 odometry, then the closures
    assert [(ctx.fa[f], ctx.fb[f]) for f in cand] == CLOSURES[:2]
    r = ctx.g.optimize_gnc(ctx.p, cand)
    assert r["chi2_final"] == ctx.g.chi2()
    ctx.p.destroy(); ctx.g.destroy()


# ---- 2. the two conventions are one code path -------------------------------------------------------------------------------------------
def test_lm_objective_is_twice_chi2_on_a_graph_of_binary_factors(lib):
    """every term of a graph without unary factors is an exact half under CHI2 (plain and robust alike) and the two sums have one tree:
    F_initial == 2 chi2 to the bit.  (No prior, no fixed node: LM's damping alone anchors the one iteration)"""
    from aprilsam_amd import datasets
    states, fa, fb, z, W = datasets.random_pose_graph(300, 200, 11)
    keep = np.asarray(fb) >= 0
    plain = tuple(np.asarray(v)[keep] for v in (fa, fb, z, W))
    F = len(plain[0])
    closures = np.nonzero(np.abs(plain[1] - plain[0]) != 1)[0]
    assert F > 300 and len(closures) >= 6
    kinds, cs = np.zeros(F, np.int32), np.ones(F)
    kinds[closures[:3]], cs[closures[:3]] = robust_model.HUBER, 0.5
    kinds[closures[3:6]], cs[closures[3:6]] = robust_model.CAUCHY, 1.0
    g = robust_model.build(lib, states, plain, kinds, cs); p = lib.new_param()
    chi2 = g.chi2()
    F0 = g.optimize_lm(p, max_iters=1)["F_initial"]
    assert chi2 > 0 and F0 == 2.0 * chi2, (F0, chi2)
    p.destroy(); g.destroy()


# ---- 3, 4. the two-stage forms of the reducer -------------------------------------------------------------------------------------------
def _lattice(lib, side):
    g = lib.new_graph()
    nfac = lib.dll.aprilsam_amd_make_lattice(g.ptr, side)
    return g, nfac


@pytest.fixture(scope="module")
def lattice316(lib):
    """(states, plain) of the 316 x 316 lattice: 99 856 poses, 397 531 factors.  Read back once, never changed"""
    g, nfac = _lattice(lib, 316)
    assert nfac == 397531
    x, fa, fb, z, W = g.arrays()
    g.destroy()
    return x, (fa, fb, z, W)


def _lm_terms(x, plain):
    fa, fb, z, W = plain
    _, _, r = linearise(x, fa, fb, z)
    return np.einsum("ni,nij,nj->n", r, np.asarray(W, float).reshape(-1, 3, 3), r)


def _F_initial_twice(lib, side):
    out = []
    for _ in range(2):
        g, _ = _lattice(lib, side); p = lib.new_param()
        out.append(g.optimize_lm(p, max_iters=1)["F_initial"])
        p.destroy(); g.destroy()
    return out


def test_lm_sums_a_large_graph_in_two_stages(lib, lattice316):
    """LM's F above 65 536 factors (k_reduce_parts + k_reduce through enqueue_reduce): the exactly rounded sum of the model's terms to
    the bound april_graph_chi2 meets on the same graph, and the same bits on every call"""
    x, plain = lattice316
    assert len(plain[0]) > REDUCE_SPLIT
    want = math.fsum(_lm_terms(x, plain))
    F = _F_initial_twice(lib, 316)
    print("F_initial", F[0], "fsum", want, "relative", abs(F[0] - want) / want)
    assert F[0] == F[1]
    assert abs(F[0] - want) <= SUM_RTOL * want


def test_lm_sums_a_graph_below_the_split_in_one_stage(lib):
    g, nfac = _lattice(lib, 100)
    assert 0 < nfac <= REDUCE_SPLIT
    x, *plain = g.arrays()
    g.destroy()
    want = math.fsum(_lm_terms(x, plain))
    F = _F_initial_twice(lib, 100)
    print("F_initial", F[0], "fsum", want, "relative", abs(F[0] - want) / want)
    assert F[0] == F[1]
    assert abs(F[0] - want) <= SUM_RTOL * want


def test_gnc_takes_the_largest_s_of_many_candidates_in_two_stages(lib, lattice316):
    """s_max over more than 65 536 candidates (k_gnc_max_parts + k_gnc_max): a maximum adds no rounding of its own, so the bound is
    that of one evaluation of s"""
    x, plain = lattice316
    cand = np.nonzero(plain[1] >= 0)[0].astype(np.int32)
    assert len(cand) > REDUCE_SPLIT
    g, _ = _lattice(lib, 316); p = lib.new_param()
    r = g.optimize_gnc(p, cand, max_stages=1, max_iters=1)
    want = float(np.max(robust_model.s_of(x, plain)[cand]))
    print("s_max", r["s_max"], "model", want, "relative", abs(r["s_max"] - want) / want)
    assert abs(r["s_max"] - want) <= TERM_RTOL * want
    p.destroy(); g.destroy()
