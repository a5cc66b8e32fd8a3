"""Range, bearing and range-bearing factors restated in numpy / scipy on the TRUE m-row factors -- no xyt slot
anywhere in this file.  TEST INFRASTRUCTURE.

A graph is `plain` = (fa, fb, z, W) arrays of xyt / xytpos factors (tests/support/lm_model.py) plus `polars`, a list of
(kind, a, b, z [m], W [m, m]): a observes b.  q = R(theta_a)' (p_b - p_a), rho = |q|, beta = atan2(q1, q0); the residual is z - h(q), the
bearing wrapped; the Jacobians are dh/dq times the first two rows of the xyt factor's.  At rho^2 == 0 the Jacobians are zero.
F(x) = sum r' W r over all factors (LM's objective); chi2 is april_graph_chi2's: 0.5 r'Wr for xyt, r'Wr for priors and polar factors.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.support import lm_model
from tests.support.normal_eq import linearise, mod2pi

RANGE, BEARING, RANGE_BEARING = 1, 2, 3
NO_PLAIN = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros((0, 9)))


def rows(kind):
    return 2 if kind == RANGE_BEARING else 1


def rel(pa, pb):
    """q [2], dq/dpa [2, 3], dq/dpb [2, 3]"""
    c, s = np.cos(pa[2]), np.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    q = np.array([c * dx + s * dy, -s * dx + c * dy])
    Ja = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy]])
    Jb = np.array([[c, s, 0.0], [-s, c, 0.0]])
    return q, Ja, Jb


def h(kind, q):
    rho, beta = np.hypot(q[0], q[1]), np.arctan2(q[1], q[0])
    return np.array([rho]) if kind == RANGE else np.array([beta]) if kind == BEARING else np.array([rho, beta])


def G(kind, q):
    """dh/dq [m, 2]; zeros at rho^2 == 0"""
    rho2 = q[0] * q[0] + q[1] * q[1]
    if rho2 == 0:
        return np.zeros((rows(kind), 2))
    rho = np.sqrt(rho2)
    gr, gb = np.array([q[0] / rho, q[1] / rho]), np.array([-q[1] / rho2, q[0] / rho2])
    return gr[None] if kind == RANGE else gb[None] if kind == BEARING else np.vstack([gr, gb])


def residual(kind, z, q):
    r = np.asarray(z, float).ravel()[:rows(kind)] - h(kind, q)
    if kind != RANGE:
        r[-1] = mod2pi(r[-1])
    return r


def evaluate(x, pol):
    """(J_a [m, 3], J_b [m, 3], r [m], W [m, m]) of one polar factor at the states x"""
    kind, a, b, z, W = pol
    q, Ja, Jb = rel(x[a], x[b])
    g = G(kind, q)
    m = rows(kind)
    return g @ Ja, g @ Jb, residual(kind, z, q), np.asarray(W, float).reshape(m, m)


def polar_cost(x, polars):
    t = 0.0
    for pol in polars:
        _, _, r, W = evaluate(x, pol)
        t += float(r @ W @ r)
    return t


def cost(x, plain, polars):
    """LM's objective F(x)"""
    return lm_model.cost(x, plain) + polar_cost(x, polars)


def chi2(x, plain, polars):
    """april_graph_chi2: 0.5 r'Wr for xyt factors, r'Wr for xytpos priors and for polar factors"""
    fa, fb, z, W = plain
    _, _, r = linearise(x, fa, fb, z)
    t = np.einsum("ni,nij,nj->n", r, np.asarray(W, float).reshape(-1, 3, 3), r)
    return float(np.sum(np.where(np.asarray(fb) >= 0, 0.5 * t, t))) + polar_cost(x, polars)


def system(x, plain, polars, lam):
    """(A, B): sum J'WJ + lam I (sparse csc) and sum J'W r over the plain and the polar factors at x"""
    N = len(x)
    fa, fb, z, W = plain
    if len(fa):
        A, B = lm_model.system(x, fa, fb, z, W, lam)
    else:
        A, B = lam * sp.identity(3 * N, format="csc"), np.zeros(3 * N)
    ri, ci, vi = [], [], []
    for pol in polars:
        Ja, Jb, r, W = evaluate(x, pol)
        a, b = pol[1], pol[2]
        for (n0, J0) in ((a, Ja), (b, Jb)):
            B[3 * n0:3 * n0 + 3] += J0.T @ W @ r
            for (n1, J1) in ((a, Ja), (b, Jb)):
                M = J0.T @ W @ J1
                ii, jj = np.meshgrid(3 * n0 + np.arange(3), 3 * n1 + np.arange(3), indexing="ij")
                ri.append(ii.ravel()); ci.append(jj.ravel()); vi.append(M.ravel())
    if vi:
        A = (A + sp.coo_matrix((np.concatenate(vi), (np.concatenate(ri), np.concatenate(ci))), shape=(3 * N, 3 * N))).tocsc()
    return A, B


def gn_step(x, plain, polars, lam):
    """one april_graph_cholesky step from x: (dx [N, 3], new states)"""
    A, B = system(x, plain, polars, lam)
    dx = spla.spsolve(A.tocsc(), B)
    return dx.reshape(-1, 3), lm_model.retract(np.array(x, float), dx)


def gn_steps(x, plain, polars, steps, lam):
    x = np.array(x, float, copy=True)
    for _ in range(steps):
        _, x = gn_step(x, plain, polars, lam)
    return x


def pred(x, hh, plain, polars):
    """LM's model decrease sum d' W (2 r - d), d = J_a h_a + J_b h_b"""
    fa, fb, z, W = plain
    t = float(np.sum(lm_model.pred_terms(x, hh, fa, fb, z, W))) if len(fa) else 0.0
    hh = np.asarray(hh, float).reshape(-1, 3)
    for pol in polars:
        Ja, Jb, r, Wp = evaluate(x, pol)
        d = Ja @ hh[pol[1]] + Jb @ hh[pol[2]]
        t += float(d @ Wp @ (2.0 * r - d))
    return t


def _lm_loop(x0, cost_fn, system_fn, pred_fn, max_iters=50, lambda0=1e-4, lambda_max=1e16, eta=0.0, ftol=1e-10, xtol=1e-10):
    """lm_model.optimize's loop (Nielsen's rule, the stop tests and their latch) on cost_fn(x), system_fn(x, lam) -> (A, B), pred_fn(x, h)"""
    x = np.array(x0, float, copy=True)
    F = cost_fn(x)
    F0, lam, nu = F, lambda0, 2.0
    status, it, accepted = 0, 0, 0
    trace, xs, dx = [], [], None
    while status == 0:
        A, B = system_fn(x, lam)
        hv = spla.spsolve(A, B)
        rejected = bool(np.isnan(hv).any())
        xt = lm_model.retract(x, hv)
        Ft = cost_fn(xt) if not rejected else np.nan
        rejected = rejected or not np.isfinite(Ft)
        pr = pred_fn(x, hv)
        hh2, xx = float(hv @ hv), float(np.sum(x * x))
        with np.errstate(all="ignore"):
            rho = (F - Ft) / pr
        acc, lam_used = 0, lam
        if not rejected and not pr > 0:
            status = lm_model.CONVERGED_F
        elif not rejected and rho > eta:
            acc = 1
            t = 2.0 * rho - 1.0
            lam = lam * max(1.0 / 3.0, 1.0 - t * t * t)
            nu = 2.0
            Fold, F = F, Ft
            x = xt; dx = hv.reshape(-1, 3).copy()
            accepted += 1
            if Fold - Ft <= ftol * abs(Fold):
                status = lm_model.CONVERGED_F
            elif np.sqrt(hh2) <= xtol * (np.sqrt(xx) + xtol):
                status = lm_model.CONVERGED_X
        else:
            lam = lam * nu
            nu = 2.0 * nu
        trace.append((Ft, rho, lam_used, acc))
        xs.append(x.copy())
        it += 1
        if status == 0 and lam > lambda_max:
            status = lm_model.STALLED
        if status == 0 and it >= max_iters:
            status = lm_model.MAX_ITERS
    return dict(status=status, iterations=it, accepted=accepted, F_initial=F0, F_final=F, lambda_final=lam, x=x, dx=dx,
                trace=np.array(trace, float).reshape(-1, 4), xs=xs)


def optimize(x0, plain, polars, **lm):
    """aprilsam_amd_optimize_lm on plain + polar factors: dict as lm_model.optimize's"""
    return _lm_loop(x0, lambda x: cost(x, plain, polars), lambda x, lam: system(x, plain, polars, lam), lambda x, hv: pred(x, hv, plain, polars), **lm)


def gnc_optimize(x0, plain, polars, cand, loss, c=None, mu_step=1.4, max_stages=100, **lm):
    """aprilsam_amd_optimize_gnc with the plain factors `cand` as candidates on a graph that also holds polar factors (never candidates):
    gnc_model.optimize's schedule, every stage the LM loop above with the candidates' surrogate weights; dict(status, stages, iterations,
    mu_initial, mu_final, s_max, F_final, x, weights, stage_trace)"""
    from tests.support import gnc_model as gm
    from tests.support import robust_model
    c = gm.C_DEFAULT if c is None else c
    cand = np.asarray(cand, np.int64)
    x = np.array(x0, float, copy=True)
    fa, fb, z, _ = plain
    s_max = float(np.max(robust_model.s_of(x, plain)[cand]))
    mu, _ = gm.mu_start(loss, c, s_max)
    mu0, status, rows, iterations = mu, 0, [], 0
    lm = dict(dict(max_iters=10), **lm)
    while status == 0:
        def weighted(xx, mu=mu):
            return (fa, fb, z, gm.w_eff(xx, plain, cand, loss, c, mu)[0])
        r = _lm_loop(x, lambda xx, mu=mu: gm.cost(xx, plain, cand, loss, c, mu) + polar_cost(xx, polars),
                     lambda xx, lam: system(xx, weighted(xx), polars, lam), lambda xx, hv: pred(xx, hv, weighted(xx), polars), **lm)
        x = r["x"]
        iterations += r["iterations"]
        rows.append((mu, r["F_initial"], r["F_final"], r["iterations"]))
        if loss == gm.GM:
            done = mu == 1.0
        else:
            w = gm.weight(loss, c, mu, robust_model.s_of(x, plain)[cand])
            done = bool(np.all((w == 0.0) | (w == 1.0)))
        if done:
            status = gm.FINISHED
        elif len(rows) >= max_stages:
            status = gm.MAX_STAGES
        else:
            mu = max(1.0, mu / mu_step) if loss == gm.GM else mu * mu_step
    sc = robust_model.s_of(x, plain)[cand]
    return dict(status=status, stages=len(rows), iterations=iterations, mu_initial=mu0, mu_final=mu, s_max=s_max, F_final=rows[-1][2], x=x,
                weights=gm.weight(loss, c, mu, sc), stage_trace=np.array(rows, float).reshape(-1, 4))


# ---- the generator ---------------------------------------------------------------------------------------------------------------
ODO_W = np.diag([400.0, 400.0, 1e4])
PRIOR_W = np.diag([1e4, 1e4, 1e3])
SIGMA_RHO, SIGMA_BETA = 0.02, 0.01
TIKHANOV = 1e-4


def snake(K, L, radius=2.5, seed=0, kinds=(RANGE_BEARING, RANGE, BEARING), n_rows=None):
    """A snake path of K x K poses (n_rows x K when n_rows is given) on a unit grid with L landmarks, each seen from the poses within `radius`: noise 0.02 m / 0.01 rad on
    the polar measurements, odometry with 0.05 m / 0.01 rad, a prior on pose 0.  Landmarks are the nodes K*K .. K*K + L - 1 (ordinary xyt
    nodes: nothing observes their heading, tikhanov 1e-4 keeps the system regular).  The kinds cycle over the observations of a landmark.
    -> dict(truth, start (dead-reckoned poses, landmarks from their first observation), plain, polars, n_poses, events): events[i] lists
    what arrives with pose i -- ("node", id) / ("plain", index into plain) / ("polar", index into polars) -- for incremental runs."""
    rng = np.random.default_rng(seed)
    n_rows = K if n_rows is None else n_rows
    n = n_rows * K
    truth = np.zeros((n + L, 3))
    for r in range(n_rows):
        for c in range(K):
            i = r * K + (K - 1 - c if r & 1 else c)
            truth[i] = (c, r, np.pi if r & 1 else 0.0)
    for i in range(n - 1):          # headings along the path: the pose looks where it goes next (the turn at a row's end included)
        d = truth[i + 1, :2] - truth[i, :2]
        truth[i, 2] = np.arctan2(d[1], d[0])
    truth[n - 1, 2] = truth[n - 2, 2]
    truth[n:, :2] = rng.uniform([-0.5, -0.5], [K - 0.5, n_rows - 0.5], (L, 2)) + rng.choice([-0.37, 0.41], (L, 2))
    fa, fb, z, W = [0], [-1], [truth[0] + rng.normal(0, [0.01, 0.01, 0.03])], [PRIOR_W.reshape(9)]
    events = [[("node", 0), ("plain", 0)]] + [[] for _ in range(n - 1)]
    start = truth.copy()
    start[0] = z[0]
    for i in range(1, n):
        q, _, _ = rel(truth[i - 1], truth[i])
        zz = np.array([q[0], q[1], mod2pi(truth[i, 2] - truth[i - 1, 2])]) + rng.normal(0, [0.05, 0.05, 0.01])
        fa.append(i - 1); fb.append(i); z.append(zz); W.append(ODO_W.reshape(9))
        c, s = np.cos(start[i - 1, 2]), np.sin(start[i - 1, 2])
        start[i] = (start[i - 1, 0] + c * zz[0] - s * zz[1], start[i - 1, 1] + s * zz[0] + c * zz[1], mod2pi(start[i - 1, 2] + zz[2]))
        events[i] += [("node", i), ("plain", len(fa) - 1)]
    polars, seen = [], np.zeros(L, int)
    for i in range(n):
        for l in range(L):
            q, _, _ = rel(truth[i], truth[n + l])
            if np.hypot(*q) > radius:
                continue
            kind = kinds[seen[l] % len(kinds)] if seen[l] else RANGE_BEARING      # (the first sighting fixes the landmark: range and bearing)
            zz = h(RANGE_BEARING, q) + rng.normal(0, [SIGMA_RHO, SIGMA_BETA])
            if not seen[l]:
                c, s = np.cos(start[i, 2] + zz[1]), np.sin(start[i, 2] + zz[1])
                start[n + l] = (start[i, 0] + zz[0] * c, start[i, 1] + zz[0] * s, 0.0)
                events[i].append(("node", n + l))
            seen[l] += 1
            if kind == RANGE:
                pol = (RANGE, i, n + l, zz[:1].copy(), np.array([[1 / SIGMA_RHO ** 2]]))
            elif kind == BEARING:
                pol = (BEARING, i, n + l, zz[1:].copy(), np.array([[1 / SIGMA_BETA ** 2]]))
            else:
                cr = 0.3 / (SIGMA_RHO * SIGMA_BETA)          # (correlated range / bearing noise: the off-diagonal entry of W is exercised)
                pol = (RANGE_BEARING, i, n + l, zz.copy(), np.array([[1 / SIGMA_RHO ** 2, cr], [cr, 1 / SIGMA_BETA ** 2]]))
            polars.append(pol)
            events[i].append(("polar", len(polars) - 1))
    assert seen.min() > 0, "a landmark is seen from nowhere: raise the radius"
    plain = (np.array(fa, np.int64), np.array(fb, np.int64), np.array(z), np.array(W))
    return dict(truth=truth, start=start, plain=plain, polars=polars, n_poses=n, events=events)


def with_landmarks(truth, start, L, radius=2.5, seed=0):
    """L landmarks around the poses `truth` [n, 3], each seen as a range-bearing factor (noise 0.02 m / 0.01 rad) from the poses within
    `radius`: -> (truth [n + L, 3], start [n + L, 3] -- the landmarks placed by their first sighting from the pose's START --, polars)"""
    rng = np.random.default_rng(seed)
    n = len(truth)
    lo, hi = truth[:, :2].min(0) - 0.5, truth[:, :2].max(0) + 0.5
    xt = np.vstack([truth, np.column_stack([rng.uniform(lo, hi, (L, 2)) + rng.choice([-0.37, 0.41], (L, 2)), np.zeros(L)])])
    x0 = np.vstack([start, np.zeros((L, 3))])
    polars, seen = [], np.zeros(L, bool)
    for i in range(n):
        for l in range(L):
            q, _, _ = rel(xt[i], xt[n + l])
            if np.hypot(*q) > radius:
                continue
            zz = h(RANGE_BEARING, q) + rng.normal(0, [SIGMA_RHO, SIGMA_BETA])
            if not seen[l]:
                x0[n + l, :2] = x0[i, :2] + zz[0] * np.array([np.cos(x0[i, 2] + zz[1]), np.sin(x0[i, 2] + zz[1])])
                seen[l] = True
            polars.append((RANGE_BEARING, i, n + l, zz, np.diag([1 / SIGMA_RHO ** 2, 1 / SIGMA_BETA ** 2])))
    assert seen.all(), "a landmark is seen from nowhere: raise the radius"
    return xt, x0, polars


def build(lib, states, plain, polars):
    """the library's graph of (plain, polars) at `states`: plain factors first, in order, then the polar factors, in order"""
    g = lib.new_graph()
    for s in states:
        g.add_node_xyt(s)
    fa, fb, z, W = plain
    for a, b, zz, WW in zip(fa, fb, z, W):
        if b < 0:
            g.add_factor_xytpos(int(a), zz, WW)
        else:
            g.add_factor_xyt(int(a), int(b), zz, WW)
    for kind, a, b, zz, WW in polars:
        g.add_factor_polar(kind, a, b, zz, WW)
    return g
