"""Per-factor audit (include/aprilsam_amd.h: aprilsam_amd_factor_audit), dense numpy.  TEST INFRASTRUCTURE: the
restatement tests/test_gpu_factor_audit.py compares with, pinned by tests/test_audit_model.py on the CPU.

A factor is a tuple (a, b, J_a [m, 3], J_b [m, 3] or None for a prior, r [m], W [m, m]) at the linearisation point -- m = 3 for xyt /
xytpos factors (normal_eq.linearise), m = 1 or 2 for a polar factor in its TRUE form (polar_model.evaluate: no xyt slot here; the library
audits the slot, and the two agree because J_eff' W_eff J_eff = J_p' W_p J_p and G r_eff = r_p).  With Sigma the (conditional) covariance of
the system that was factorised -- exact zeros in the rows and columns of fixed nodes -- and Delta its step:

    v = r - J Delta_f        P = J Sigma_ff J'        M = I - P W
    chi2 = v' W v    leverage = tr(P W)    d2_loo = v' W M^-1 v  (NaN when det M <= 0 or not finite)    checkability = det M

Tolerances: the project's SIG_RTOL (1e-9 of row_scale(Sigma), tests/support/sigma_compare.py) pushed through these formulas to first order:
an error E in Sigma_ff with |E_ij| <= SIG_RTOL * scale moves tr(P W) = tr(Sigma_ff J' W J) by at most SIG_RTOL * scale * sum |J' W J|."""
import numpy as np

from tests.support import fixed_model
from tests.support.normal_eq import linearise
from tests.support.selinv_model import dense_system, system_blocks
from tests.support.sigma_compare import SIG_RTOL, row_scale

CHI2_RTOL = 1e-12                # no Sigma involved
CHECK_FLOOR = 1e-3               # d2_loo is compared only where the model's checkability is at least this


def xyt_factors(lp, fa, fb, z, W):
    """the factor tuples of plain (fa, fb, z, W) arrays at lp (fb < 0: xytpos prior)"""
    Ja, Jb, r = linearise(lp, fa, fb, z)
    W = np.asarray(W, float).reshape(-1, 3, 3)
    return [(int(fa[f]), int(fb[f]), Ja[f], Jb[f] if fb[f] >= 0 else None, r[f], W[f]) for f in range(len(fa))]


def polar_factors(lp, polars):
    """the factor tuples of polar factors (tests/support/polar_model.py) at lp, in their m-row form"""
    from tests.support import polar_model
    out = []
    for pol in polars:
        Ja, Jb, r, W = polar_model.evaluate(lp, pol)
        out.append((int(pol[1]), int(pol[2]), Ja, Jb, r, W))
    return out


def dense_A(lp, factors, lam):
    """A = sum J' W J + lam I, dense [3N, 3N] in node order"""
    N = len(lp)
    A = lam * np.eye(3 * N)
    for a, b, Ja, Jb, r, W in factors:
        ix = np.r_[3 * a:3 * a + 3] if Jb is None else np.r_[3 * a:3 * a + 3, 3 * b:3 * b + 3]
        J = Ja if Jb is None else np.hstack([Ja, Jb])
        A[np.ix_(ix, ix)] += J.T @ W @ J
    return A


def dense_B(lp, factors):
    B = np.zeros(3 * len(lp))
    for a, b, Ja, Jb, r, W in factors:
        B[3 * a:3 * a + 3] += Ja.T @ W @ r
        if Jb is not None:
            B[3 * b:3 * b + 3] += Jb.T @ W @ r
    return B


def solve(A, B, fixed=()):
    """(Sigma, Delta [N, 3]) of the system with `fixed` held constant: the conditional covariance (zeros at fixed nodes) and the step"""
    Sig = fixed_model.conditional_covariance(A, fixed) if len(fixed) else np.linalg.inv(A)
    d = fixed_model.reduced_solve(A, B, fixed) if len(fixed) else np.linalg.solve(A, B)
    return Sig, d.reshape(-1, 3)


def block(Sig, a, b):
    ix = np.r_[3 * a:3 * a + 3] if b is None or b < 0 else np.r_[3 * a:3 * a + 3, 3 * b:3 * b + 3]
    return Sig[np.ix_(ix, ix)]


def one(Sff, d, fac):
    """(chi2, leverage, d2_loo, checkability) of one factor from its nodes' block of Sigma and their steps d (3 or 6)"""
    a, b, Ja, Jb, r, W = fac
    J = Ja if Jb is None else np.hstack([Ja, Jb])
    v = r - J @ d
    P = J @ Sff @ J.T
    M = np.eye(len(r)) - P @ W
    det = float(np.linalg.det(M))
    d2 = float(v @ W @ np.linalg.solve(M, v)) if det > 0 and np.isfinite(det) else np.nan
    return np.array([float(v @ W @ v), float(np.trace(P @ W)), d2, det])


def audit(Sig, Delta, factors):
    """[F, 4] of every factor from the dense Sigma and the step Delta [N, 3]"""
    Delta = np.asarray(Delta, float).reshape(-1, 3)
    out = np.empty((len(factors), 4))
    for i, fac in enumerate(factors):
        a, b = fac[0], fac[1]
        d = Delta[a] if fac[3] is None else np.r_[Delta[a], Delta[b]]
        out[i] = one(block(Sig, a, b if fac[3] is not None else None), d, fac)
    return out


def tolerances(Sig, factors, model):
    """[F, 4] per factor: relative for chi2 (column 0) and d2_loo (column 2; relative to max(d2_loo, chi2), inf below CHECK_FLOOR), absolute
    for leverage and checkability.  `model`: audit()'s result"""
    scale = row_scale(Sig)
    tol = np.empty((len(factors), 4))
    for i, (a, b, Ja, Jb, r, W) in enumerate(factors):
        J = Ja if Jb is None else np.hstack([Ja, Jb])
        sc = scale[a] if Jb is None else max(scale[a], scale[b])
        lev = SIG_RTOL * sc * float(np.abs(J.T @ W @ J).sum())
        det = model[i, 3]
        # (every node of the factor fixed: Sigma_ff = 0 exactly, the Sigma bound is 0 and d2_loo IS chi2: chi2's own tolerance)
        tol[i] = (CHI2_RTOL, lev, (lev / det if lev > 0 else CHI2_RTOL) if det >= CHECK_FLOOR else np.inf, 3.0 * lev)
    return tol


def _ratio(diff, tol):
    """diff / tol; 0 where diff is exactly 0 (a tolerance of 0 -- every node of the factor fixed -- asks for the model's bits)"""
    with np.errstate(all="ignore"):
        r = np.asarray(diff, float) / tol
    return np.where(diff == 0, 0.0, r)


def compare(got, model, tol):
    """assert the library's rows against the model's within `tol`; returns (worst ratios [4], number of factors below the floor)"""
    got = np.asarray(got, float); model = np.asarray(model, float)
    assert got.shape == model.shape, (got.shape, model.shape)
    worst = np.zeros(4)
    ref = np.maximum(np.abs(model[:, 0]), 1e-300)
    worst[0] = _ratio(np.abs(got[:, 0] - model[:, 0]), tol[:, 0] * ref).max()
    for k in (1, 3):
        worst[k] = _ratio(np.abs(got[:, k] - model[:, k]), tol[:, k]).max()
    hi = model[:, 3] >= CHECK_FLOOR
    if hi.any():
        ref2 = np.maximum(np.maximum(model[hi, 2], model[hi, 0]), 1e-300)
        worst[2] = _ratio(np.abs(got[hi, 2] - model[hi, 2]), tol[hi, 2] * ref2).max()
    lo = got[~hi, 2]
    assert np.all(np.isnan(lo) | (np.isfinite(lo) & (lo >= 0))), lo      # below the floor: NaN, or finite and not negative
    assert np.all(worst <= 1.0), worst
    return worst, int((~hi).sum())


def polar_chi2_allowance(chi2, z_eff, W_eff):
    """What the slot form costs a polar factor's chi2 against its TRUE m-row form -- a statement about two numpy models, never a bound on the
    library, which is held to the model of the slot it reads.  The slot stores a MEASUREMENT, z_eff = q + r_eff (csrc/polar.h), and the kernels
    take the residual back as z_eff - q: r_eff comes back with the rounding of a number of z_eff's size, not of its own.  Four such
    roundings separate the library's v from the model's -- the slot's sum and the kernel's difference, and on the model's side h(q) and
    z - h(q) -- so v differs by d with |d_i| <= 4 eps |z_eff_i| (eps = 2^-52), and chi2 = v' W v by at most 2 sqrt(chi2 d' W d) + d' W d
    (Cauchy-Schwarz in the W_eff inner product).  A factor whose post-fit residual is 1e-3 of its measurement loses three digits this way;
    for an xyt factor the same term exists but z is the relative pose itself and the observed error stays under 1e-12."""
    d = 4.0 * 2.0 ** -52 * np.abs(np.asarray(z_eff, float))
    dWd = float(d @ np.abs(np.asarray(W_eff, float).reshape(3, 3)) @ d)
    return 2.0 * np.sqrt(max(float(chi2), 0.0) * dWd) + dWd


def trace_identity(audit_rows, Sig_diag, lam, n_free):
    """sum of the leverages + sum_i lam_i tr(Sigma_ii) - 3 n_free (zero: tr(Sigma A) = 3 N).  Sig_diag [N, 3, 3]; lam scalar or [N]"""
    lam = np.broadcast_to(np.asarray(lam, float), (len(Sig_diag),))
    return float(np.nansum(audit_rows[:, 1]) + np.sum(lam * np.trace(Sig_diag, axis1=1, axis2=2)) - 3.0 * n_free)


# ---- the two sides of the leave-one-out identity in extended precision ----------------------------------------------------------------
# For a factor that nothing else checks (a lone prior: det M ~ lambda^3 / det W) both sides lose digits in double -- M = I - P W cancels to
# 1e-6, the reduced system's condition number is ~1e9 -- and agree to 1e-9 only by luck (random_0's prior: 1.3e-9 apart in double, and 2.7e-10
# apart with refined solves of the double-rounded A).  Here the system is FORMED and solved in numpy's longdouble (Jacobians, J' W J, the
# Cholesky solves refined against longdouble residuals, the m x m algebra), so the identity itself is what the test sees.
LD = np.longdouble


def _factors_ld(lp, fa, fb, z, W):
    lp = np.asarray(lp, LD).reshape(-1, 3); z = np.asarray(z, LD).reshape(-1, 3); W = np.asarray(W, LD).reshape(-1, 3, 3)
    pi = np.arctan2(LD(0), LD(-1)); twopi = 2 * pi
    out = []
    for f in range(len(fa)):
        a, b = int(fa[f]), int(fb[f])
        if b < 0:
            r = z[f] - lp[a]
            Ja, Jb = np.eye(3, dtype=LD), None
        else:
            pa, pb = lp[a], lp[b]
            c, s = np.cos(pa[2]), np.sin(pa[2])
            dx, dy = pb[0] - pa[0], pb[1] - pa[1]
            Ja = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0, 0, -1]], LD)
            Jb = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], LD)
            r = np.array([z[f, 0] - (c * dx + s * dy), z[f, 1] - (-s * dx + c * dy), z[f, 2] - (pb[2] - pa[2])], LD)
        r[2] = (r[2] + pi) - twopi * np.floor((r[2] + pi) / twopi) - pi
        out.append((a, b, Ja, Jb, r, W[f]))
    return out


def _solve_ld(A, R, free):
    """X with A[free, free] X[free] = R[free] (zeros elsewhere), longdouble: double Cholesky, refined against longdouble residuals"""
    import scipy.linalg as sl
    Af = A[np.ix_(free, free)]
    c = sl.cho_factor(Af.astype(float))
    X = sl.cho_solve(c, R[free].astype(float)).astype(LD)
    for _ in range(5):
        X = X + sl.cho_solve(c, (R[free] - Af @ X).astype(float)).astype(LD)
    out = np.zeros(R.shape, LD)
    out[free] = X
    return out


def _small_solve_ld(M, v):
    """Gaussian elimination with partial pivoting in longdouble (numpy.linalg has none)"""
    M = np.array(M, LD); v = np.array(v, LD); n = len(v)
    for i in range(n):
        p = i + int(np.argmax(np.abs(M[i:, i])))
        M[[i, p]] = M[[p, i]]; v[[i, p]] = v[[p, i]]
        for j in range(i + 1, n):
            t = M[j, i] / M[i, i]; M[j] = M[j] - t * M[i]; v[j] = v[j] - t * v[i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (v[i] - M[i, i + 1:] @ x[i + 1:]) / M[i, i]
    return x


def identity_sides(lp, fa, fb, z, W, lam, f, fixed=()):
    """(d2_loo, e' S^-1 e) of factor f of a plain graph at lp: v' W M^-1 v from the full system, and f gated against the system without it"""
    facs = _factors_ld(lp, fa, fb, z, W)
    N3 = 3 * len(np.asarray(lp).reshape(-1, 3))
    free = np.setdiff1d(np.arange(N3), fixed_model.dofs(fixed)) if len(fixed) else np.arange(N3)
    a, b, Ja, Jb, r, Wf = facs[f]
    J = Ja if Jb is None else np.hstack([Ja, Jb])
    ix = np.r_[3 * a:3 * a + 3] if Jb is None else np.r_[3 * a:3 * a + 3, 3 * b:3 * b + 3]
    E = np.zeros((N3, len(ix)), LD); E[ix, np.arange(len(ix))] = 1

    def sides(factors):
        A = LD(lam) * np.eye(N3, dtype=LD); B = np.zeros(N3, LD)
        for a_, b_, Ja_, Jb_, r_, W_ in factors:
            jx = np.r_[3 * a_:3 * a_ + 3] if Jb_ is None else np.r_[3 * a_:3 * a_ + 3, 3 * b_:3 * b_ + 3]
            J_ = Ja_ if Jb_ is None else np.hstack([Ja_, Jb_])
            A[np.ix_(jx, jx)] += J_.T @ W_ @ J_
            B[jx] += J_.T @ W_ @ r_
        X = _solve_ld(A, np.column_stack([E, B]), free)
        return X[ix, :len(ix)], X[ix, len(ix)]
    Sff, d = sides(facs)
    v = r - J @ d
    M = np.eye(3, dtype=LD) - J @ Sff @ J.T @ Wf
    d2 = v @ Wf @ _small_solve_ld(M, v)
    Sff1, d1 = sides([fc for i, fc in enumerate(facs) if i != f])
    e = r - J @ d1
    Winv = np.column_stack([_small_solve_ld(Wf, np.eye(3, dtype=LD)[:, k]) for k in range(3)])
    S = J @ Sff1 @ J.T + Winv
    return d2, e @ _small_solve_ld(S, e)


def graph_model(lp, fa, fb, z, W, lam, Delta=None, fixed=()):
    """(rows [F, 4], tol [F, 4], Sig, factors) of a plain xyt / xytpos graph at lp; Delta: the step to audit with (default: the model's own)"""
    lp = np.asarray(lp, float).reshape(-1, 3)
    facs = xyt_factors(lp, fa, fb, z, W)
    Aii, Aab = system_blocks(lp, fa, fb, z, W, lam)
    A = dense_system(Aii, Aab, fa, fb)
    Sig, d = solve(A, dense_B(lp, facs), fixed)
    rows = audit(Sig, d if Delta is None else Delta, facs)
    return rows, tolerances(Sig, facs, rows), Sig, facs
