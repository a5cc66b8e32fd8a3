"""Robust losses on xyt / xytpos factors, restated in numpy / scipy.  TEST INFRASTRUCTURE.

A graph is `plain` = (fa, fb, z, W) arrays (fb < 0: xytpos prior) plus per factor a loss kind (0 none, 1 Huber, 2 Cauchy, 3 DCS) and a
scale c.  With s = r' W r (r the plain residual, theta wrapped):
    rho(s)  Huber: s <= c^2 ? s : 2 c sqrt(s) - c^2;  Cauchy: c^2 log1p(s / c^2);  DCS: s <= c^2 ? s : c^2 (3 s - c^2) / (s + c^2)
    w(s)    = rho'(s)
Every linearisation uses W_eff = w(s) W at the linearisation point (IRLS).  april_graph_chi2 counts 0.5 rho for xyt, rho for xytpos;
the LM objective counts rho.  The Gauss-Newton / LM machinery is lm_model's."""
import ctypes as C
import os
import subprocess

import numpy as np
import scipy.sparse.linalg as spla

from aprilsam_amd import abi
from tests.support import lm_model, maxmix_model
from tests.support.normal_eq import linearise

ROOT = maxmix_model.ROOT
NONE, HUBER, CAUCHY, DCS = abi.ROBUST_NONE, abi.ROBUST_HUBER, abi.ROBUST_CAUCHY, abi.ROBUST_DCS


def rho(kind, c, s):
    s = np.asarray(s, float)
    kind = np.broadcast_to(kind, s.shape); c = np.broadcast_to(np.asarray(c, float), s.shape)
    cc = c * c
    with np.errstate(all="ignore"):
        out = np.where(kind == HUBER, np.where(s <= cc, s, 2.0 * c * np.sqrt(s) - cc), s)
        out = np.where(kind == CAUCHY, cc * np.log1p(s / cc), out)
        out = np.where(kind == DCS, np.where(s <= cc, s, cc * (3.0 * s - cc) / (s + cc)), out)
    return out


def weight(kind, c, s):
    s = np.asarray(s, float)
    kind = np.broadcast_to(kind, s.shape); c = np.broadcast_to(np.asarray(c, float), s.shape)
    cc = c * c
    with np.errstate(all="ignore"):
        out = np.where(kind == HUBER, np.where(s <= cc, 1.0, c / np.sqrt(s)), 1.0)
        out = np.where(kind == CAUCHY, 1.0 / (1.0 + s / cc), out)
        out = np.where(kind == DCS, np.where(s <= cc, 1.0, 4.0 * cc * cc / ((s + cc) * (s + cc))), out)
    return out


def s_of(x, plain):
    """per factor s = r' W r at x (xytpos at x too: the batch and LM steps linearise priors at the state, which equals l_point)"""
    fa, fb, z, W = plain
    _, _, r = linearise(x, fa, fb, z)
    W = np.asarray(W, float).reshape(-1, 3, 3)
    return np.einsum("ni,nij,nj->n", r, W, r)


def weights(x, plain, kind, c):
    return weight(kind, c, s_of(x, plain))


def w_eff(x, plain, kind, c):
    """(W_eff [F, 9], w [F]): one multiply per entry, as the library forms it"""
    w = weights(x, plain, kind, c)
    return w[:, None] * np.asarray(plain[3], float).reshape(-1, 9), w


def chi2(x, plain, kind, c):
    """april_graph_chi2 of a robust graph"""
    rh = rho(kind, c, s_of(x, plain))
    return float(np.sum(np.where(np.asarray(plain[1]) >= 0, 0.5 * rh, rh)))


def cost(x, plain, kind, c):
    """the LM objective F = sum rho(s)"""
    return float(np.sum(rho(kind, c, s_of(x, plain))))


def irls_steps(x, plain, kind, c, steps, lam=1e-4):
    """`steps` reference batch steps (Tikhonov lam on every pose) with W_eff at each step's point: the list of states after each"""
    x = np.array(x, float, copy=True)
    fa, fb, z, _ = plain
    out = []
    for _ in range(steps):
        We, _ = w_eff(x, plain, kind, c)
        A, B = lm_model.system(x, fa, fb, z, We, lam)
        x = lm_model.retract(x, spla.spsolve(A, B))
        out.append(x.copy())
    return out


def optimize(x0, plain, kind, c, max_iters=50, lambda0=1e-4, lambda_max=1e16, eta=0.0, ftol=1e-10, xtol=1e-10):
    """aprilsam_amd_optimize_lm on a robust graph: lm_model.optimize with W_eff at each iteration's point and F = sum rho"""
    x = np.array(x0, float, copy=True)
    fa, fb, z, _ = plain
    F = cost(x, plain, kind, c)
    F0, lam, nu = F, lambda0, 2.0
    status, it, accepted = 0, 0, 0
    trace, xs, preds = [], [], []
    while status == 0:
        We, _ = w_eff(x, plain, kind, c)
        A, B = lm_model.system(x, fa, fb, z, We, lam)
        h = spla.spsolve(A, B)
        rejected = bool(np.isnan(h).any())
        xt = lm_model.retract(x, h)
        Ft = cost(xt, plain, kind, c) if not rejected else np.nan
        rejected = rejected or not np.isfinite(Ft)
        pred = float(np.sum(lm_model.pred_terms(x, h, fa, fb, z, We)))
        preds.append((pred, float(h @ B), float(h @ h), lam))
        hh, xx = float(h @ h), float(np.sum(x * x))
        with np.errstate(all="ignore"):
            rr = (F - Ft) / pred
        acc = 0
        lam_used = lam
        if not rejected and not pred > 0:
            status = lm_model.CONVERGED_F
        elif not rejected and rr > eta:
            acc = 1
            t = 2.0 * rr - 1.0
            lam = lam * max(1.0 / 3.0, 1.0 - t * t * t)
            nu = 2.0
            Fold, F = F, Ft
            x = xt
            accepted += 1
            if Fold - Ft <= ftol * abs(Fold):
                status = lm_model.CONVERGED_F
            elif np.sqrt(hh) <= xtol * (np.sqrt(xx) + xtol):
                status = lm_model.CONVERGED_X
        else:
            lam = lam * nu
            nu = 2.0 * nu
        trace.append((Ft, rr, lam_used, acc))
        xs.append(x.copy())
        it += 1
        if status == 0 and lam > lambda_max:
            status = lm_model.STALLED
        if status == 0 and it >= max_iters:
            status = lm_model.MAX_ITERS
    return dict(status=status, iterations=it, accepted=accepted, F_initial=F0, F_final=F, lambda_final=lam, x=x,
                trace=np.array(trace, float).reshape(-1, 4), xs=xs, preds=preds)


# ---- scenarios ---------------------------------------------------------------------------------------------------------------
def m3500_robust(kind, c, n_out=50, seed=7):
    """maxmix_model.m3500_outliers as one plain array set: (states, plain, kinds, cs, n_base, n_loops): the odometry chain + prior first
    (no loss), then the loop closures and the false ones, all with loss `kind` and scale c"""
    states, base, loops, outl = maxmix_model.m3500_outliers(n_out, seed)
    edges = loops + outl
    fa = np.concatenate([base[0], [e[0] for e in edges]]).astype(np.int32)
    fb = np.concatenate([base[1], [e[1] for e in edges]]).astype(np.int32)
    z = np.concatenate([np.asarray(base[2]).reshape(-1, 3), np.array([e[2] for e in edges]).reshape(-1, 3)])
    W = np.concatenate([np.asarray(base[3]).reshape(-1, 9), np.array([np.asarray(e[3]).reshape(9) for e in edges])])
    nb = len(base[0])
    kinds = np.zeros(len(fa), np.int32); kinds[nb:] = kind
    cs = np.zeros(len(fa)); cs[nb:] = c
    return states, (fa, fb, z, W), kinds, cs, nb, len(loops)


def build(lib, states, plain, kinds, cs):
    """a product graph from the arrays, the losses set with Graph.set_robust"""
    g = lib.new_graph()
    g.build_from_arrays(states, *plain)
    for i in np.nonzero(np.asarray(kinds) != NONE)[0]:
        assert g.set_robust(int(i), int(kinds[i]), float(cs[i])) == 0
    return g


def build_helper_lib(outdir):
    """compile tests/support/robust_factor.c (the independent checker) and bind it"""
    out = os.path.join(outdir, "librobust_factor.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "support", "robust_factor.c"), "-o", out, "-lm"])
    cl = C.CDLL(out)
    cl.rb_create.restype = C.POINTER(abi.Factor)
    cl.rb_create.argtypes = [C.c_int, C.POINTER(abi.Factor), C.c_int, C.c_double]
    cl.rb_last_w.argtypes = [C.POINTER(abi.Factor)]
    cl.rb_last_w.restype = C.c_double
    cl.rb_evals.restype = C.c_longlong
    return cl


def build_checker(lib, cl, states, plain, kinds, cs, type_tag=99, upto=None):
    """a graph of `lib` (the reference, typically) with every robust factor wrapped in the checker factor over lib's own xyt factor"""
    g = lib.new_graph()
    fa, fb, z, W = plain
    F = len(fa) if upto is None else upto
    for i in range(len(states)):
        g.add_node_xyt(states[i])
    for i in range(F):
        add_factor(lib, cl, g, fa[i], fb[i], z[i], W[i], kinds[i], cs[i], type_tag)
    return g


def add_factor(lib, cl, g, a, b, z, W, kind, c, type_tag=99):
    m = g._matd(W)
    zz = (C.c_double * 3)(*z)
    if b < 0:
        f = lib.dll.april_graph_factor_xytpos_create(int(a), zz, None, C.byref(m))
    else:
        f = lib.dll.april_graph_factor_xyt_create(int(a), int(b), zz, None, C.byref(m))
    if kind != NONE:
        f = cl.rb_create(int(type_tag), f, int(kind), float(c))
    lib._add_factor(g.ptr, f)
