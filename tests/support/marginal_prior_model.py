"""Dense numpy model of DESIGN.md section 24: the dense Gaussian factor on k nodes (information form) and the marginal prior that
eliminating a node set leaves on its Markov blanket.  TEST INFRASTRUCTURE (a checker, like oracle/): never used by the product package.

Everything is written against a dtype: the tests run it in float64 and again in np.longdouble on the same input, and take ten times the
difference of the two as the deviation they allow the library (the rule of the section; the figures are recorded there).

    linearise_t         tests/support/normal_eq.py's Jacobians and residuals, every operation in the dtype (the longdouble model is longdouble
                        from the poses on: what the float64 evaluation of a sine loses is part of the deviation, as it is of the device's)
    dense_system        H = sum J'WJ, g = sum J'W r of xyt / xytpos factors at lp, dense, in node order
    gaussian_delta      delta = x (-) xbar per node, headings wrapped with mod2pi
    gaussian_system     the factor's H = Lambda, g = eta - Lambda delta, added into a dense system
    pivoted_cholesky    diagonally pivoted Cholesky with LAPACK dpstrf's default stop; sqrt_form: R, d, c0 with R'R = Lambda, R'd = eta
    gaussian_chi2       c0 - 2 eta'delta + delta'Lambda delta
    solve_spd           Gaussian elimination without pivoting in the dtype at hand (np.linalg knows no longdouble)
    marginal_prior      keep (the blanket, ascending), Lambda = H_BB - H_BM H_MM^-1 H_MB, eta = g_B - H_BM H_MM^-1 g_M from the factors that
                        touch M only
"""
import numpy as np

from tests.support.normal_eq import linearise, TWOPI


def mod2pi(v, dtype=np.float64):
    v = np.asarray(v, dtype)
    pi = dtype(np.pi); twopi = dtype(TWOPI)          # (the library's constants are doubles)
    vin = v + pi
    return vin - twopi * np.floor(vin / twopi) - pi


def linearise_t(lp, fa, fb, z, dtype=np.float64):
    """tests/support/normal_eq.py's linearise (J_a, J_b, r per factor at lp) with every operation -- the sines and cosines included -- in
    dtype: in float64 it IS that function, in longdouble it is the reference the float64 evaluation deviates from"""
    if dtype is np.float64:
        return linearise(lp, fa, fb, z)
    lp = np.asarray(lp, dtype).reshape(-1, 3); z = np.asarray(z, dtype).reshape(-1, 3)
    fa = np.asarray(fa); fb = np.asarray(fb)
    F = len(fa)
    binary = fb >= 0
    pa = lp[fa]; pb = lp[np.where(binary, fb, 0)]
    ca, sa = np.cos(pa[:, 2]), np.sin(pa[:, 2])
    dx, dy = pb[:, 0] - pa[:, 0], pb[:, 1] - pa[:, 1]
    Ja = np.zeros((F, 3, 3), dtype); Jb = np.zeros((F, 3, 3), dtype); r = np.zeros((F, 3), dtype)
    Ja[:, 0, 0] = -ca; Ja[:, 0, 1] = -sa; Ja[:, 0, 2] = -sa * dx + ca * dy
    Ja[:, 1, 0] = sa;  Ja[:, 1, 1] = -ca; Ja[:, 1, 2] = -ca * dx - sa * dy
    Ja[:, 2, 2] = -1
    Jb[:, 0, 0] = ca;  Jb[:, 0, 1] = sa
    Jb[:, 1, 0] = -sa; Jb[:, 1, 1] = ca
    Jb[:, 2, 2] = 1
    r[:, 0] = z[:, 0] - (ca * dx + sa * dy)
    r[:, 1] = z[:, 1] - (-sa * dx + ca * dy)
    r[:, 2] = mod2pi(z[:, 2] - (pb[:, 2] - pa[:, 2]), dtype)
    u = ~binary
    if u.any():
        Ja[u] = np.eye(3, dtype=dtype); Jb[u] = 0
        r[u, 0] = z[u, 0] - pa[u, 0]; r[u, 1] = z[u, 1] - pa[u, 1]; r[u, 2] = mod2pi(z[u, 2] - pa[u, 2], dtype)
    return Ja, Jb, r


def dense_system(lp, fa, fb, z, W, dtype=np.float64, only=None, upt=None):
    """(H [3N, 3N], g [3N]) of the xyt / xytpos factors (those listed in `only`, all by default) at lp; priors at upt (lp by default)"""
    lp = np.asarray(lp, float).reshape(-1, 3)
    N = len(lp)
    fa = np.asarray(fa, np.int64); fb = np.asarray(fb, np.int64)
    z = np.asarray(z, float).reshape(-1, 3); W = np.asarray(W, float).reshape(-1, 3, 3)
    H = np.zeros((3 * N, 3 * N), dtype); g = np.zeros(3 * N, dtype)
    Ja, Jb, r = linearise_t(lp, fa, fb, z, dtype)
    if upt is not None:
        u = fb < 0
        _, _, ru = linearise_t(np.asarray(upt, float).reshape(-1, 3), fa, fb, z, dtype)
        r[u] = ru[u]
    for f in (range(len(fa)) if only is None else only):
        a, b = int(fa[f]), int(fb[f])
        Wf = W[f].astype(dtype); A = Ja[f].astype(dtype); B = Jb[f].astype(dtype); rf = r[f].astype(dtype)
        H[3 * a:3 * a + 3, 3 * a:3 * a + 3] += A.T @ Wf @ A
        g[3 * a:3 * a + 3] += A.T @ (Wf @ rf)
        if b >= 0:
            H[3 * b:3 * b + 3, 3 * b:3 * b + 3] += B.T @ Wf @ B
            H[3 * a:3 * a + 3, 3 * b:3 * b + 3] += A.T @ Wf @ B
            H[3 * b:3 * b + 3, 3 * a:3 * a + 3] += (A.T @ Wf @ B).T
            g[3 * b:3 * b + 3] += B.T @ (Wf @ rf)
    return H, g


def gaussian_delta(pts, nodes, xbar, dtype=np.float64):
    pts = np.asarray(pts, dtype).reshape(-1, 3); xbar = np.asarray(xbar, dtype).reshape(-1, 3)
    d = pts[np.asarray(nodes, np.int64)] - xbar
    d[:, 2] = mod2pi(d[:, 2], dtype)
    return d.reshape(-1)


def _rows(nodes):
    return np.array([3 * int(n) + c for n in nodes for c in range(3)], np.int64)


def gaussian_system(H, g, pts, nodes, xbar, eta, Lam):
    """add the factor's H = Lambda and g = eta - Lambda delta (delta at pts) into the dense system, in its dtype"""
    dtype = H.dtype.type
    L = np.asarray(Lam, dtype); d = gaussian_delta(pts, nodes, xbar, dtype)
    rows = _rows(nodes)
    H[np.ix_(rows, rows)] += L
    g[rows] += np.asarray(eta, dtype) - L @ d
    return H, g


def pivoted_cholesky(Lam, dtype=np.float64):
    """(R [rank, n] with R'R = Lambda in the ORIGINAL column order, rank): diagonal pivoting, the first of equal candidates; stop when the
    largest remaining diagonal <= n eps(float64) max diag (dpstrf's default, the library's rule -- the SAME bound in either dtype)"""
    A = np.array(Lam, dtype); n = len(A)
    Rp = np.zeros((n, n), dtype); piv = np.arange(n)
    amax = max(float(np.max(np.diag(A))) if n else 0.0, 0.0)
    tol = n * np.finfo(np.float64).eps * amax
    rank = 0
    for j in range(n):
        p = j + int(np.argmax(np.diag(A)[j:]))
        if not A[p, p] > tol:
            break
        if p != j:
            A[:, [j, p]] = A[:, [p, j]]; A[[j, p], :] = A[[p, j], :]
            Rp[:j, [j, p]] = Rp[:j, [p, j]]
            piv[[j, p]] = piv[[p, j]]
        Rp[j, j] = np.sqrt(A[j, j])
        Rp[j, j + 1:] = A[j, j + 1:] / Rp[j, j]
        A[j + 1:, j + 1:] -= np.outer(Rp[j, j + 1:], Rp[j, j + 1:])
        rank = j + 1
    R = np.zeros((rank, n), dtype)
    R[:, piv] = Rp[:rank, :]
    return R, rank, piv, Rp[:rank]


def sqrt_form(eta, Lam, dtype=np.float64):
    """(R, d, c0): R'R = Lambda, R'd = eta from the triangular solve in pivot order, c0 = d'd"""
    R, rank, piv, Rp = pivoted_cholesky(Lam, dtype)
    e = np.asarray(eta, dtype)[piv]
    d = np.zeros(rank, dtype)
    for l in range(rank):
        d[l] = (e[l] - Rp[:l, l] @ d[:l]) / Rp[l, l]
    return R, d, d @ d


def gaussian_chi2(pts, nodes, xbar, eta, Lam, c0, dtype=np.float64):
    d = gaussian_delta(pts, nodes, xbar, dtype)
    L = np.asarray(Lam, dtype); e = np.asarray(eta, dtype)
    return dtype(c0) - 2 * (e @ d) + d @ (L @ d)


def solve_spd(A, B, dtype=np.float64):
    """A^-1 B by Gaussian elimination without pivoting (A symmetric positive definite), in dtype"""
    A = np.array(A, dtype); X = np.array(B, dtype)
    vec = X.ndim == 1
    if vec:
        X = X[:, None]
    n = len(A)
    for j in range(n):
        if not A[j, j] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} = {A[j, j]} is not positive")
        f = A[j + 1:, j] / A[j, j]
        A[j + 1:, j:] -= np.outer(f, A[j, j:])
        X[j + 1:] -= np.outer(f, X[j])
    for j in range(n - 1, -1, -1):
        X[j] = (X[j] - A[j, j + 1:] @ X[j + 1:]) / A[j, j]
    return X[:, 0] if vec else X


def blanket(fa, fb, remove):
    """(F_M: the factors with an endpoint in M, B: their other endpoints, ascending)"""
    M = set(int(i) for i in remove)
    FM = [f for f in range(len(fa)) if int(fa[f]) in M or int(fb[f]) in M]
    B = sorted({int(x) for f in FM for x in (fa[f], fb[f]) if x >= 0 and int(x) not in M})
    return FM, B


def schur(H, g, remove, keep):
    """(Lambda, eta) on `keep` after eliminating `remove` from the dense system, in its dtype"""
    dtype = H.dtype.type
    m, b = _rows(remove), _rows(keep)
    if len(m) == 0:
        return H[np.ix_(b, b)].copy(), g[b].copy()
    X = solve_spd(H[np.ix_(m, m)], np.concatenate([H[np.ix_(m, b)], g[m][:, None]], axis=1), dtype)
    L = H[np.ix_(b, b)] - H[np.ix_(b, m)] @ X[:, :-1]
    return (L + L.T) / 2, g[b] - H[np.ix_(b, m)] @ X[:, -1]


def marginal_prior(lp, fa, fb, z, W, remove, dtype=np.float64, extra=None, extra_nodes=(), upt=None):
    """(keep, xbar [|B|, 3], eta, Lambda) of eliminating `remove`: H and g from the xyt / xytpos factors that touch M only (plus
    extra(H, g): a callback that adds the contributions of further factors that touch M, e.g. a Gaussian factor's, whose nodes outside
    M are listed in extra_nodes)"""
    FM, B = blanket(fa, fb, remove)
    B = sorted(set(B) | {int(x) for x in extra_nodes if int(x) not in set(int(i) for i in remove)})
    H, g = dense_system(lp, fa, fb, z, W, dtype, only=FM, upt=upt)
    if extra is not None:
        extra(H, g)
    L, e = schur(H, g, list(remove), B)
    return np.array(B, np.int32), np.asarray(lp, float).reshape(-1, 3)[B].copy(), e, L
