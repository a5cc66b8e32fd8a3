"""Graduated non-convexity as aprilsam_amd_optimize_gnc runs it, restated in numpy / scipy.  TEST INFRASTRUCTURE.

A graph is `plain` = (fa, fb, z, W) arrays (fb < 0: xytpos prior); `cand` lists the factors the surrogate applies to.  With s = r' W r of
the plain factor, cc = c^2 and the control parameter mu:
    GM   m = mu cc:  rho = m s / (m + s),  w = (m / (m + s))^2
    TLS  lo = mu / (mu + 1) cc, hi = (mu + 1) / mu cc:  s <= lo: rho = s, w = 1;  s >= hi: rho = cc, w = 0;
         otherwise rho = 2 c sqrt(mu (mu + 1) s) - mu (cc + s),  w = c sqrt(mu (mu + 1) / s) - mu;  mu = inf: lo = hi = cc (TLS itself)
A stage is lm_model's iteration loop with W_eff = w_mu(s) W on the candidates at every linearisation and rho_mu(s) in the objective,
lambda restarting at lambda0.  The schedule: GM starts at mu = max(1, 2 s_max / cc) and divides by mu_step down to 1; TLS starts at
cc / (2 s_max - cc) and multiplies until every weight is 0 or 1."""
import numpy as np
import scipy.sparse.linalg as spla

from tests.support import lm_model, robust_model

GM, TLS = 1, 2
FINISHED, MAX_STAGES = 1, 2
C_DEFAULT = float(np.sqrt(16.27))


def _bounds(c, mu):
    cc = c * c
    if np.isinf(mu):
        return cc, cc
    return mu / (mu + 1.0) * cc, (mu + 1.0) / mu * cc


def weight(loss, c, mu, s):
    s = np.asarray(s, float)
    cc = c * c
    with np.errstate(all="ignore"):
        if loss == GM:
            m = mu * cc
            q = m / (m + s)
            return q * q
        lo, hi = _bounds(c, mu)
        mid = c * np.sqrt(mu * (mu + 1.0) / s) - mu
        return np.where(s <= lo, 1.0, np.where(s >= hi, 0.0, mid))


def rho(loss, c, mu, s):
    s = np.asarray(s, float)
    cc = c * c
    with np.errstate(all="ignore"):
        if loss == GM:
            m = mu * cc
            return m * s / (m + s)
        lo, hi = _bounds(c, mu)
        mid = 2.0 * c * np.sqrt(mu * (mu + 1.0) * s) - mu * (cc + s)
        return np.where(s <= lo, s, np.where(s >= hi, cc, mid))


def mu_start(loss, c, s_max):
    """(mu0, all_inliers)"""
    cc = c * c
    if loss == GM:
        return max(1.0, 2.0 * s_max / cc), False
    if 2.0 * s_max > cc:
        return cc / (2.0 * s_max - cc), False
    return float("inf"), True


def cost(x, plain, cand, loss, c, mu):
    s = robust_model.s_of(x, plain)
    s[cand] = rho(loss, c, mu, s[cand])
    return float(np.sum(s))


def w_eff(x, plain, cand, loss, c, mu):
    w = np.ones(len(plain[0]))
    w[cand] = weight(loss, c, mu, robust_model.s_of(x, plain)[cand])
    return w[:, None] * np.asarray(plain[3], float).reshape(-1, 9), w


def stage(x0, plain, cand, loss, c, mu, max_iters=10, lambda0=1e-4, lambda_max=1e16, eta=0.0, ftol=1e-10, xtol=1e-10):
    """one stage: robust_model.optimize's loop with the surrogate of mu on the candidates"""
    x = np.array(x0, float, copy=True)
    fa, fb, z, _ = plain
    F = cost(x, plain, cand, loss, c, mu)
    F0, lam, nu = F, lambda0, 2.0
    status, it, accepted = 0, 0, 0
    trace, dx = [], None
    while status == 0:
        We, _ = w_eff(x, plain, cand, loss, c, mu)
        A, B = lm_model.system(x, fa, fb, z, We, lam)
        h = spla.spsolve(A, B)
        rejected = bool(np.isnan(h).any())
        xt = lm_model.retract(x, h)
        Ft = cost(xt, plain, cand, loss, c, mu) if not rejected else np.nan
        rejected = rejected or not np.isfinite(Ft)
        pred = float(np.sum(lm_model.pred_terms(x, h, fa, fb, z, We)))
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
            x = xt; dx = h.reshape(-1, 3).copy()
            accepted += 1
            if Fold - Ft <= ftol * abs(Fold):
                status = lm_model.CONVERGED_F
            elif np.sqrt(hh) <= xtol * (np.sqrt(xx) + xtol):
                status = lm_model.CONVERGED_X
        else:
            lam = lam * nu
            nu = 2.0 * nu
        trace.append((Ft, rr, lam_used, acc))
        it += 1
        if status == 0 and lam > lambda_max:
            status = lm_model.STALLED
        if status == 0 and it >= max_iters:
            status = lm_model.MAX_ITERS
    return dict(status=status, iterations=it, accepted=accepted, F_initial=F0, F_final=F, x=x, dx=dx, trace=np.array(trace, float).reshape(-1, 4))


def optimize(x0, plain, cand, loss, c=C_DEFAULT, mu_step=1.4, max_stages=100, **lm):
    """the device's run: dict(status, stages, iterations, accepted, stages_stalled, n_inliers, mu_initial, mu_final, s_max, F_final, x,
    dx, weights, s, stage_trace [stages, 4] (mu, F on entry, F at the end, LM iterations), lm_traces: each stage's LM trace and entry F)"""
    cand = np.asarray(cand, np.int64)
    x = np.array(x0, float, copy=True)
    cc = c * c
    s_max = float(np.max(robust_model.s_of(x, plain)[cand]))
    mu, _ = mu_start(loss, c, s_max)
    mu0 = mu
    status, rows, lm_traces, dx = 0, [], [], None
    iterations = accepted = stalled = 0
    while status == 0:
        r = stage(x, plain, cand, loss, c, mu, **lm)
        x = r["x"]
        if r["dx"] is not None:
            dx = r["dx"]
        iterations += r["iterations"]; accepted += r["accepted"]; stalled += r["status"] == lm_model.STALLED
        rows.append((mu, r["F_initial"], r["F_final"], r["iterations"]))
        lm_traces.append((r["F_initial"], r["trace"]))
        if loss == GM:
            done = mu == 1.0
        else:
            w = weight(loss, c, mu, robust_model.s_of(x, plain)[cand])
            done = bool(np.all((w == 0.0) | (w == 1.0)))
        if done:
            status = FINISHED
        elif len(rows) >= max_stages:
            status = MAX_STAGES
        else:
            mu = max(1.0, mu / mu_step) if loss == GM else mu * mu_step
    s = robust_model.s_of(x, plain)[cand]
    return dict(status=status, stages=len(rows), iterations=iterations, accepted=accepted, stages_stalled=int(stalled),
                n_inliers=int(np.sum(s <= cc)), mu_initial=mu0, mu_final=mu, s_max=s_max, F_final=rows[-1][2], x=x, dx=dx,
                weights=weight(loss, c, mu, s), s=s, stage_trace=np.array(rows, float).reshape(-1, 4), lm_traces=lm_traces)


# ---- scenarios ---------------------------------------------------------------------------------------------------------------
CASES = [(4, 3, 3), (6, 6, 3), (6, 10, 5)]
SIGMA_XY, SIGMA_T = 0.02, 0.01


def _measure(pa, pb):
    ca, sa = np.cos(pa[2]), np.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    return np.array([ca * dx + sa * dy, -sa * dx + ca * dy, lm_model.mod2pi(pb[2] - pa[2])])


def _compose(pa, z):
    ca, sa = np.cos(pa[2]), np.sin(pa[2])
    return np.array([pa[0] + ca * z[0] - sa * z[1], pa[1] + sa * z[0] + ca * z[1], lm_model.mod2pi(pa[2] + z[2])])


def snake(K, n_out, seed):
    """the issue's scenario: dict(truth, start, plain, cand (every closure), is_false (per candidate))
    A snake path over a K x K unit grid (row 0 left to right, row 1 right to left, ...), headings along the direction of travel; a prior
    on pose 0, odometry, closures between vertically adjacent cells that are not consecutive on the path, every measurement with noise
    sigma 0.02 in x and y and 0.01 rad; n_out false closures between uniformly random distinct non-consecutive poses with a uniformly
    random measurement; the start is the dead-reckoned odometry."""
    rng = np.random.default_rng(seed)
    N = K * K
    cell = lambda i: ((i % K) if (i // K) % 2 == 0 else K - 1 - (i % K), i // K)
    index = {cell(i): i for i in range(N)}
    truth = np.zeros((N, 3))
    for i in range(N):
        truth[i, :2] = cell(i)
    for i in range(N):
        j = i + 1 if i + 1 < N else i - 1
        d = (truth[j, :2] - truth[i, :2]) * (1.0 if j > i else -1.0)
        truth[i, 2] = np.arctan2(d[1], d[0])
    sig = np.array([SIGMA_XY, SIGMA_XY, SIGMA_T])
    W = np.diag(1.0 / sig ** 2).reshape(9)
    fa, fb, z = [0], [-1], [truth[0].copy()]
    start = [truth[0].copy()]
    for i in range(N - 1):
        zi = _measure(truth[i], truth[i + 1]) + rng.normal(0.0, sig)
        fa.append(i); fb.append(i + 1); z.append(zi)
        start.append(_compose(start[-1], zi))
    n_base = len(fa)
    for row in range(K - 1):
        for col in range(K):
            a, b = index[(col, row)], index[(col, row + 1)]
            if abs(a - b) > 1:
                fa.append(min(a, b)); fb.append(max(a, b)); z.append(_measure(truth[min(a, b)], truth[max(a, b)]) + rng.normal(0.0, sig))
    n_true = len(fa) - n_base
    for _ in range(n_out):
        while True:
            a, b = (int(v) for v in rng.integers(0, N, 2))
            if abs(a - b) > 1:
                break
        fa.append(a); fb.append(b)
        z.append(np.array([rng.uniform(-K, K), rng.uniform(-K, K), rng.uniform(-np.pi, np.pi)]))
    F = len(fa)
    plain = (np.array(fa, np.int32), np.array(fb, np.int32), np.array(z, float).reshape(-1, 3), np.tile(W, (F, 1)))
    cand = np.arange(n_base, F, dtype=np.int32)
    is_false = np.arange(n_base, F) >= n_base + n_true
    return dict(truth=truth, start=np.array(start), plain=plain, cand=cand, is_false=is_false)


def position_error(x, truth):
    return float(np.max(np.linalg.norm(np.asarray(x)[:, :2] - np.asarray(truth)[:, :2], axis=1)))


_runs = {}


def model_run(case, loss):
    """the model's run of a case with the default options, computed once per process and shared (do not modify)"""
    key = (tuple(case), loss)
    if key not in _runs:
        sc = snake(*case)
        _runs[key] = optimize(sc["start"], sc["plain"], sc["cand"], loss)
    return _runs[key]
