"""Levenberg-Marquardt as aprilsam_amd_optimize_lm runs it, restated in numpy / scipy.  TEST INFRASTRUCTURE.

A graph is `plain` = (fa, fb, z, W) arrays (fb < 0: xytpos prior) plus `mixes`, a list of max factors (a, b, zs, Ws, logw).  The
objective is F(x) = sum_f r_f' W_f r_f (no 0.5), a max factor contributing min_k (r_k' W_k r_k + c_k), c_k = -2 logw_k - ln det W_k.
Each iteration selects the max-factor components at x, solves (sum J'WJ + lambda I) h = sum J'W r with spsolve, forms
x_t = x (+) h (theta wrapped), the model decrease pred = sum_f d_f' W_f (2 r_f - d_f), and applies Nielsen's rule and the stop tests
with the device's latch.

With spd_check (a function: dense matrix -> the pivots of its LDL' without pivoting; the tests pass pivot_placement.ldl_pivots) the model also
takes the device's other rejection (k_lm_decide: `not_spd`): a system sum J'WJ + lambda I with a non-positive
pivot is not solved, the step is rejected (lambda <- lambda nu, nu <- 2 nu) and counted in rejected_not_spd.  Positive definiteness is decided
by the sign of the smallest pivot of a dense LDL' (tests/support/pivot_placement.py: by Sylvester's law the count of negative pivots does not
depend on the elimination order); `margins` records min_j |d_j| / A_jj per iteration, so that a test can keep every decision away from
rounding.  The model eliminates in NODE order, the device in its plan's order: the sign of the decision is the same, the margin is not --
each pivot of the other order has its own size -- so a margin says how far THIS order's decision is from rounding, and the tests ask for one
thousands of times the float64 pivot error (pivot_placement.LM_MARGIN) to leave room for the other.
Dense, O(n^3) per iteration: for graphs of a few hundred unknowns.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.support import maxmix_model
from tests.support.normal_eq import linearise, mod2pi

CONVERGED_F, CONVERGED_X, STALLED, MAX_ITERS = 1, 2, 3, 4


def perturbed(states, sigma, seed=1):
    """the start of the issue's runs: every heading + N(0, sigma^2) from default_rng(seed)"""
    x = np.array(states, float, copy=True)
    x[:, 2] += np.random.default_rng(seed).normal(0.0, sigma, len(x))
    return x


def _quad(W, v):
    W = W.reshape(-1, 3, 3)
    return np.einsum("ni,nij,nj->n", v, W, v)


def mix_const(Ws, logw):
    return np.array([-2.0 * lw - np.log(np.linalg.det(np.asarray(W, float).reshape(3, 3))) for W, lw in zip(Ws, logw)])


def selected(x, mixes):
    """plain arrays of the components selected at x (maxmix_model.select: lowest score, lower index on a tie)"""
    fa, fb, z, W = [], [], [], []
    for a, b, zs, Ws, lw in mixes:
        s = maxmix_model.select(x[a], x[b], zs, Ws, lw)
        fa.append(a); fb.append(b); z.append(np.asarray(zs[s], float)); W.append(np.asarray(Ws[s], float).reshape(9))
    return (np.array(fa, np.int64), np.array(fb, np.int64), np.array(z).reshape(-1, 3), np.array(W).reshape(-1, 9))


def cost(x, plain, mixes=()):
    """F(x)"""
    fa, fb, z, W = plain
    _, _, r = linearise(x, fa, fb, z)
    total = float(np.sum(_quad(np.asarray(W, float), r)))
    for a, b, zs, Ws, lw in mixes:
        c = mix_const(Ws, lw)
        total += min(maxmix_model.rtwr(np.asarray(Ws[k], float).reshape(9), maxmix_model.residual(x[a], x[b], zs[k])) + c[k] for k in range(len(zs)))
    return total


def _concat(plain, extra):
    if extra is None or len(extra[0]) == 0:
        return tuple(np.asarray(v) for v in plain)
    return tuple(np.concatenate([np.asarray(p), np.asarray(e)]) for p, e in zip(plain, extra))


def system(x, fa, fb, z, W, lam):
    """(A, B): sum J'WJ + lam I (sparse, 3N x 3N) and sum J'W r at x"""
    N = len(x)
    fa = np.asarray(fa, np.int64); fb = np.asarray(fb, np.int64); W = np.asarray(W, float).reshape(-1, 3, 3)
    Ja, Jb, r = linearise(x, fa, fb, z)
    binary = fb >= 0
    rows, cols, vals = [], [], []
    B = np.zeros(3 * N)

    def block(Jl, Jr, il, ir, mask):
        M = np.einsum("nki,nkl,nlj->nij", Jl[mask], W[mask], Jr[mask])
        ii = 3 * il[mask][:, None, None] + np.arange(3)[None, :, None]
        jj = 3 * ir[mask][:, None, None] + np.arange(3)[None, None, :]
        rows.append(np.broadcast_to(ii, M.shape).ravel()); cols.append(np.broadcast_to(jj, M.shape).ravel()); vals.append(M.ravel())

    allm = np.ones(len(fa), bool)
    fbb = np.where(binary, fb, 0)
    block(Ja, Ja, fa, fa, allm)
    block(Ja, Jb, fa, fbb, binary)
    block(Jb, Ja, fbb, fa, binary)
    block(Jb, Jb, fbb, fbb, binary)
    Wr = np.einsum("nij,nj->ni", W, r)
    ga = np.einsum("nki,nk->ni", Ja, Wr); gb = np.einsum("nki,nk->ni", Jb, Wr)
    for k in range(3):
        B[k::3] += np.bincount(fa, weights=ga[:, k], minlength=N) + np.bincount(fbb, weights=gb[:, k] * binary, minlength=N)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * N, 3 * N)).tocsc()
    if lam:
        A = A + lam * sp.identity(3 * N, format="csc")
    return A, B


def pred_terms(x, h, fa, fb, z, W):
    """per factor d' W (2 r - d), d = J_a h_a + J_b h_b at x"""
    fa = np.asarray(fa, np.int64); fb = np.asarray(fb, np.int64); W = np.asarray(W, float).reshape(-1, 3, 3)
    h = np.asarray(h, float).reshape(-1, 3)
    Ja, Jb, r = linearise(x, fa, fb, z)
    binary = fb >= 0
    d = np.einsum("nij,nj->ni", Ja, h[fa]) + np.einsum("nij,nj->ni", Jb, h[np.where(binary, fb, 0)]) * binary[:, None]
    return np.einsum("ni,nij,nj->n", d, W, 2.0 * r - d)


def retract(x, h):
    xt = x + h.reshape(-1, 3)
    xt[:, 2] = mod2pi(x[:, 2] + h.reshape(-1, 3)[:, 2])
    return xt


def gn_steps(x, plain, steps, lam=0.0, mixes=()):
    """plain Gauss-Newton with the fixed damping lam: [F(x_0), ..., F(x_steps)] and the final x"""
    x = np.array(x, float, copy=True)
    Fs = [cost(x, plain, mixes)]
    for _ in range(steps):
        fa, fb, z, W = _concat(plain, selected(x, mixes) if mixes else None)
        A, B = system(x, fa, fb, z, W, lam)
        h = spla.spsolve(A, B)
        x = retract(x, h)
        Fs.append(cost(x, plain, mixes))
    return np.array(Fs), x


def optimize(x0, plain, mixes=(), max_iters=50, lambda0=1e-4, lambda_max=1e16, eta=0.0, ftol=1e-10, xtol=1e-10, spd_check=False):
    """the device's run: dict(status, iterations, accepted, rejected_not_spd, F_initial, F_final, lambda_final, x, dx, trace [it, 4], xs: x
    after every iteration, margins: see the module docstring (spd_check only)); spd_check: None / False, or the pivots function"""
    x = np.array(x0, float, copy=True)
    F = cost(x, plain, mixes)
    F0, lam, nu = F, lambda0, 2.0
    status, it, accepted = 0, 0, 0
    trace, xs, dx = [], [], None
    rejected_not_spd, margins = 0, []
    while status == 0:
        fa, fb, z, W = _concat(plain, selected(x, mixes) if mixes else None)
        A, B = system(x, fa, fb, z, W, lam)
        not_spd = False
        if spd_check:
            Ad = A.toarray()
            d = spd_check(Ad)
            not_spd = bool(np.isnan(d).any() or np.min(d) <= 0)
            margins.append(float(np.nanmin(np.abs(d) / np.abs(np.diag(Ad)))))
            rejected_not_spd += not_spd
        h = np.full(len(B), np.nan) if not_spd else spla.spsolve(A, B)
        rejected = bool(np.isnan(h).any())
        xt = retract(x, h)
        Ft = cost(xt, plain, mixes) if not rejected else np.nan
        rejected = rejected or not np.isfinite(Ft)
        pred = float(np.sum(pred_terms(x, h, fa, fb, z, W)))
        hh, xx = float(h @ h), float(np.sum(x * x))
        with np.errstate(all="ignore"):
            rho = (F - Ft) / pred
        acc = 0
        lam_used = lam
        if not rejected and not pred > 0:
            status = CONVERGED_F
        elif not rejected and rho > eta:
            acc = 1
            t = 2.0 * rho - 1.0
            lam = lam * max(1.0 / 3.0, 1.0 - t * t * t)
            nu = 2.0
            Fold, F = F, Ft
            x = xt; dx = h.reshape(-1, 3).copy()
            accepted += 1
            if Fold - Ft <= ftol * abs(Fold):
                status = CONVERGED_F
            elif np.sqrt(hh) <= xtol * (np.sqrt(xx) + xtol):
                status = CONVERGED_X
        else:
            lam = lam * nu
            nu = 2.0 * nu
        trace.append((Ft, rho, lam_used, acc))
        xs.append(x.copy())
        it += 1
        if status == 0 and lam > lambda_max:
            status = STALLED
        if status == 0 and it >= max_iters:
            status = MAX_ITERS
    return dict(status=status, iterations=it, accepted=accepted, rejected_not_spd=rejected_not_spd, margins=np.array(margins), F_initial=F0, F_final=F, lambda_final=lam, x=x, dx=dx,
                trace=np.array(trace, float).reshape(-1, 4), xs=xs)


def comparable_rows(trace, F_before=None, eta=0.0, f_band=1e-12):
    """number of leading iterations outside the round-off band: stop at the first iteration whose |rho - eta| < 1e-6 or whose relative
    F change is below f_band (past the optimum the decisions are rounding)"""
    n = 0
    F = F_before
    for Ft, rho, lam, acc in trace:
        if not np.isfinite(rho) or abs(rho - eta) < 1e-6:
            break
        if F is not None and abs(F - Ft) <= f_band * abs(F):
            break
        if acc:
            F = Ft
        n += 1
    return n
