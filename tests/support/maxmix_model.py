"""numpy restatement of the max-mixture factor and the scenarios its tests share.

Score of component i at poses (pa, pb): s_i = r_i^T W_i r_i - 2 logw_i - ln det W_i, r_i the xyt residual (mod2pi on theta);
selection: best = 0; for i in 1..K-1: if s_i < s_best: best = i.  chi^2: 0.5 r_s^T W_s r_s for a max factor (selected at the
states), 0.5 r^T W r for xyt, r^T W r for xytpos."""
import ctypes as C
import os
import subprocess

import numpy as np

from aprilsam_amd import abi, datasets

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LN09, LN01 = float(np.log(0.9)), float(np.log(0.1))


def mod2pi(v):
    twopi, pi = 6.2831853071795862319959, 3.141592653589793238462643383279502884196
    vin = v + pi
    return (vin - twopi * np.floor(vin / twopi)) - pi


def residual(pa, pb, z):
    ca, sa = np.cos(pa[2]), np.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    return np.array([z[0] - (ca * dx + sa * dy), z[1] - (-sa * dx + ca * dy), mod2pi(z[2] - (pb[2] - pa[2]))])


def rtwr(W, r):
    w = np.asarray(W, float).reshape(9)
    X = [w[3 * i] * r[0] + w[3 * i + 1] * r[1] + w[3 * i + 2] * r[2] for i in range(3)]
    return r[0] * X[0] + r[1] * X[1] + r[2] * X[2]


def scores(pa, pb, zs, Ws, logw):
    return np.array([rtwr(W, residual(pa, pb, z)) + (-2.0 * lw - np.log(np.linalg.det(np.asarray(W, float).reshape(3, 3))))
                     for z, W, lw in zip(zs, Ws, logw)])


def select(pa, pb, zs, Ws, logw):
    s = scores(pa, pb, zs, Ws, logw)
    best = 0
    for i in range(1, len(s)):
        if s[i] < s[best]:
            best = i
    return best


def chi2(states, plain, mixes):
    """plain = (fa, fb, z, W) arrays (fb < 0: xytpos); mixes = list of (a, b, zs, Ws, logw)"""
    fa, fb, z, W = plain
    total = 0.0
    for i in range(len(fa)):
        if fb[i] < 0:
            p = states[fa[i]]
            total += rtwr(W[i], np.array([z[i][0] - p[0], z[i][1] - p[1], mod2pi(z[i][2] - p[2])]))
        else:
            total += 0.5 * rtwr(W[i], residual(states[fa[i]], states[fb[i]], z[i]))
    for a, b, zs, Ws, lw in mixes:
        s = select(states[a], states[b], zs, Ws, lw)
        total += 0.5 * rtwr(Ws[s], residual(states[a], states[b], zs[s]))
    return total


# ---- scenarios ---------------------------------------------------------------------------------------------------------------
def two_component(z, W):
    """a loop closure as the inlier {z, W, ln 0.9} against the broad null hypothesis {z, 1e-6 W, ln 0.1}"""
    W = np.asarray(W, float).reshape(9)
    return [np.asarray(z, float), np.asarray(z, float)], [W, 1e-6 * W], [LN09, LN01]


def m3500_outliers(n_out=50, seed=7):
    """M3500 with its prior; returns (states, base, loops, outliers): base = the odometry chain + prior as plain arrays
    (fa, fb, z, W), loops / outliers = lists of (a, b, z, W) -- the loop closures (|a - b| > 1) and n_out false ones"""
    states, fa, fb, z, W = datasets.m3500_batch()
    odo = (fb < 0) | (np.abs(fa - fb) <= 1)
    base = (fa[odo], fb[odo], z[odo], W[odo])
    loops = [(int(fa[i]), int(fb[i]), z[i], W[i]) for i in np.nonzero(~odo)[0]]
    rng = np.random.default_rng(seed)
    N = len(states)
    outliers = []
    while len(outliers) < n_out:
        a, b = sorted(int(v) for v in rng.integers(0, N, 2))
        if b - a <= 1:
            continue
        zz = np.array([rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(-np.pi, np.pi)])
        outliers.append((a, b, zz, loops[0][3]))
    return states, base, loops, outliers


def build(lib, states, base, edges, as_max, add_max=None):
    """a graph of `lib`: the plain arrays `base`, then every edge of `edges` as a 2-component max factor (as_max) or as a plain xyt
    factor.  add_max(g, a, b, zs, Ws, logw) makes the max factor (default: the product's Graph.add_factor_max)"""
    g = lib.new_graph()
    fa, fb, z, W = base
    g.build_from_arrays(states, fa, fb, z, W)
    for a, b, zz, WW in edges:
        if as_max:
            zs, Ws, lw = two_component(zz, WW)
            (add_max or (lambda g_, *args: g_.add_factor_max(*args)))(g, a, b, zs, Ws, lw)
        else:
            g.add_factor_xyt(a, b, zz, np.asarray(WW).reshape(3, 3))
    return g


def mixes_of(edges):
    return [(a, b) + two_component(zz, WW) for a, b, zz, WW in edges]


def build_helper_lib(outdir):
    """compile tests/support/maxmix_factor.c (the independent checker) and bind it"""
    out = os.path.join(outdir, "libmaxmix_factor.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "support", "maxmix_factor.c"), "-o", out, "-lm"])
    cl = C.CDLL(out)
    cl.mm_create.restype = C.POINTER(abi.Factor)
    cl.mm_create.argtypes = [C.c_int, C.POINTER(C.POINTER(abi.Factor)), C.POINTER(C.c_double), C.c_int]
    for nm in ("mm_last", "mm_last_state"):
        getattr(cl, nm).argtypes = [C.POINTER(abi.Factor)]
        getattr(cl, nm).restype = C.c_int
    cl.mm_min_margin.restype = C.c_double
    cl.mm_evals.restype = C.c_longlong
    return cl


def helper_adder(lib, cl, type_tag=99, record=None):
    """add_max for build(): the checker's max factor over `lib`'s own xyt components; record (a list) collects the factor pointers"""
    def add(g, a, b, zs, Ws, logw):
        K = len(zs)
        comps = (C.POINTER(abi.Factor) * K)()
        for i in range(K):
            m = g._matd(Ws[i])
            comps[i] = lib.dll.april_graph_factor_xyt_create(int(a), int(b), (C.c_double * 3)(*zs[i]), None, C.byref(m))
        f = cl.mm_create(int(type_tag), comps, (C.c_double * K)(*logw), K)
        lib._add_factor(g.ptr, f)
        if record is not None:
            record.append(f)
    return add
