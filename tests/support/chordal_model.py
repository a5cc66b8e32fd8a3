"""Chordal initialisation as aprilsam_amd_initialize_chordal computes it, restated in numpy / scipy on 2 unknowns
per pose and solved with spsolve.  TEST INFRASTRUCTURE.

A graph is `plain` = (fa, fb, z, W) arrays (fb < 0: xytpos prior), conventions of tests/support/normal_eq.py.
Stage 1 (headings): unknown u_i = (c_i, s_i); an xyt factor with w = W[2][2] > 0 contributes w |R(z_theta) u_a - u_b|^2, a prior with
w > 0 contributes w |u_a - (cos z_theta, sin z_theta)|^2; theta_i = atan2(s_i, c_i), a pose with c^2 + s^2 == 0 or a non-finite value
keeps its incoming heading.  Stage 2 (positions, headings fixed): unknown t_i; an xyt factor with W[0][0] > 0 and det Wxy > 0 contributes
|R(theta_a)' (t_b - t_a) - z_xy|^2_Wxy, a prior under the same condition |t_a - z_xy|^2_Wxy.  Damping 0 in both.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.support.normal_eq import mod2pi

ORDERINGS = ("COLAMD", "NATURAL", "MMD_AT_PLUS_A")


def _arrays(plain):
    fa, fb, z, W = plain
    return (np.asarray(fa, np.int64), np.asarray(fb, np.int64), np.asarray(z, float).reshape(-1, 3), np.asarray(W, float).reshape(-1, 3, 3))


def _rot(a):
    c, s = np.cos(a), np.sin(a)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)        # [n, 2, 2]


def choose_components(mixes):
    """plain arrays of the component each max factor (a, b, zs, Ws, logw) enters as: the largest log weight, lowest index on a tie"""
    fa, fb, z, W = [], [], [], []
    for a, b, zs, Ws, lw in mixes:
        k = int(np.argmax(np.asarray(lw, float)))
        fa.append(a); fb.append(b); z.append(np.asarray(zs[k], float)); W.append(np.asarray(Ws[k], float).reshape(9))
    return (np.array(fa, np.int64), np.array(fb, np.int64), np.array(z).reshape(-1, 3), np.array(W).reshape(-1, 9))


def _blocks(N, D, fa, fb, Haa, Hab, Hbb, ga, gb, on, pad):
    """the D-unknowns-per-pose system from per-factor d x d blocks (d = 2): A (sparse), B.  pad: D = 3, every contributing factor adds 1.0
    to element [2][2] of its diagonal blocks -- the mapping onto the 3-DoF machinery"""
    d = 2
    binary = fb >= 0
    rows, cols, vals = [], [], []

    def put(M, il, ir, mask):
        ii = D * il[mask][:, None, None] + np.arange(d)[None, :, None]
        jj = D * ir[mask][:, None, None] + np.arange(d)[None, None, :]
        rows.append(np.broadcast_to(ii, M[mask].shape).ravel()); cols.append(np.broadcast_to(jj, M[mask].shape).ravel()); vals.append(M[mask].ravel())

    fbb = np.where(binary, fb, 0)
    put(Haa, fa, fa, on)
    put(Hab, fa, fbb, on & binary)
    put(np.swapaxes(Hab, 1, 2), fbb, fa, on & binary)
    put(Hbb, fbb, fbb, on & binary)
    if pad:
        for idx in (fa[on], fb[on & binary]):
            rows.append(D * idx + 2); cols.append(D * idx + 2); vals.append(np.ones(len(idx)))
    B = np.zeros(D * N)
    for k in range(d):
        B[k::D] += np.bincount(fa[on], weights=ga[on][:, k], minlength=N) + np.bincount(fb[on & binary], weights=gb[on & binary][:, k], minlength=N)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(D * N, D * N)).tocsc()
    return A, B


def stage1_system(N, plain, pad=False):
    fa, fb, z, W = _arrays(plain)
    w = W[:, 2, 2]
    on = w > 0
    binary = fb >= 0
    I2 = np.broadcast_to(np.eye(2), (len(fa), 2, 2))
    Haa = w[:, None, None] * I2
    Hab = -w[:, None, None] * np.swapaxes(_rot(z[:, 2]), 1, 2)                # -w R(z_theta)'
    ga = np.where(binary[:, None], 0.0, w[:, None] * np.stack([np.cos(z[:, 2]), np.sin(z[:, 2])], -1))
    return _blocks(N, 3 if pad else 2, fa, fb, Haa, Hab, Haa, ga, np.zeros_like(ga), on, pad)


def stage2_system(N, plain, theta, pad=False):
    fa, fb, z, W = _arrays(plain)
    Wxy = W[:, :2, :2]
    on = (Wxy[:, 0, 0] > 0) & (np.linalg.det(Wxy) > 0)
    binary = fb >= 0
    Ra = _rot(np.where(binary, np.asarray(theta, float)[fa], 0.0))            # (priors: the identity)
    M = np.einsum("nij,njk,nlk->nil", Ra, Wxy, Ra)
    v = np.einsum("nij,njk,nk->ni", Ra, Wxy, z[:, :2])                        # R_a Wxy z_xy
    ga = np.where(binary[:, None], -v, v)
    return _blocks(N, 3 if pad else 2, fa, fb, M, -M, M, ga, v, on, pad)


def _conditions(W):
    Wxy = W[:, :2, :2]
    return W[:, 2, 2] > 0, (Wxy[:, 0, 0] > 0) & (np.linalg.det(Wxy) > 0)


def unanchored_stage(plain, N, stages=3):
    """1 / 2: the first stage with a set of poses, connected by the stage's contributing xyt factors, that none of its contributing priors
    reaches (the stage's matrix is then singular, whatever rounding makes of its pivots), or 0: what the library refuses with -2"""
    import scipy.sparse.csgraph as csg
    fa, fb, z, W = _arrays(plain)
    for stage, on in enumerate(_conditions(W)[:2 if stages == 3 else 1], start=1):
        e = on & (fb >= 0)
        G = sp.coo_matrix((np.ones(int(e.sum())), (fa[e], fb[e])), shape=(N, N))
        _, label = csg.connected_components(G, directed=False)
        if len(set(label.tolist()) - set(label[fa[on & (fb < 0)]].tolist())):
            return stage
    return 0


def initialize(plain, states_in, permc_spec="COLAMD", pad=False, stages=3):
    """dict(x [N,3]: the initial guess, u [N,2]: the stage-1 solution before normalisation, n_degenerate, min_norm, pad1 / pad2: the padded
    third unknowns when pad).  states_in: the incoming states (read for degenerate poses and for stages = 1 only)"""
    x = np.array(states_in, float, copy=True)
    N = len(x)
    D = 3 if pad else 2
    A, B = stage1_system(N, plain, pad)
    sol = spla.spsolve(A, B, permc_spec=permc_spec).reshape(N, D)
    u = sol[:, :2]
    n2 = u[:, 0] ** 2 + u[:, 1] ** 2
    ok = np.isfinite(u).all(axis=1) & np.isfinite(n2) & (n2 > 0)
    x[ok, 2] = np.arctan2(u[ok, 1], u[ok, 0])
    out = dict(u=u.copy(), n_degenerate=int(np.sum(~ok)), min_norm=float(np.sqrt(np.where(ok, n2, 0.0).min())))
    if pad:
        out["pad1"] = sol[:, 2].copy()
    if stages == 3:
        A, B = stage2_system(N, plain, x[:, 2], pad)
        sol = spla.spsolve(A, B, permc_spec=permc_spec).reshape(N, D)
        x[:, :2] = sol[:, :2]
        if pad:
            out["pad2"] = sol[:, 2].copy()
    out["x"] = x
    return out


def state_diff(a, b):
    """largest state difference, headings wrapped"""
    d = np.asarray(a, float) - np.asarray(b, float)
    d[:, 2] = mod2pi(d[:, 2])
    return float(np.abs(d).max())


def spread(plain, states_in):
    """the model's own spread: the largest state difference between the orderings spsolve offers"""
    xs = [initialize(plain, states_in, permc_spec=o)["x"] for o in ORDERINGS]
    return max(state_diff(xs[0], x) for x in xs[1:])


def residuals(plain, u, x):
    """matrix-free A u - B of stage 1 (at u [N,2]) and of stage 2 (at the positions of x, with the headings of x), each relative to the
    largest sum of |terms| of that stage's right-hand side: dict(rel1, rel2, res1, res2, scale1, scale2)"""
    fa, fb, z, W = _arrays(plain)
    u = np.asarray(u, float).reshape(-1, 2); x = np.asarray(x, float).reshape(-1, 3)
    N = len(x)
    binary = fb >= 0
    fbb = np.where(binary, fb, 0)

    def scatter(ta, tb, mask):
        out = np.zeros((N, 2))
        for k in range(2):
            out[:, k] = np.bincount(fa[mask], weights=ta[mask][:, k], minlength=N) + np.bincount(fb[mask & binary], weights=tb[mask & binary][:, k], minlength=N)
        return out

    # stage 1
    w = W[:, 2, 2]
    on = w > 0
    Rz = _rot(z[:, 2])
    zc = np.stack([np.cos(z[:, 2]), np.sin(z[:, 2])], -1)
    e = np.where(binary[:, None], np.einsum("nij,nj->ni", Rz, u[fa]) - u[fbb], u[fa] - zc)
    ta = np.where(binary[:, None], w[:, None] * np.einsum("nji,nj->ni", Rz, e), w[:, None] * e)
    res1 = scatter(ta, -w[:, None] * e, on)
    rhs = np.where(binary[:, None], 0.0, np.abs(w[:, None] * zc))
    scale1 = float(scatter(rhs, np.zeros_like(rhs), on).max())
    # stage 2
    Wxy = W[:, :2, :2]
    on = (Wxy[:, 0, 0] > 0) & (np.linalg.det(Wxy) > 0)
    Ra = _rot(np.where(binary, x[fa, 2], 0.0))
    t = x[:, :2]
    e = np.where(binary[:, None], np.einsum("nji,nj->ni", Ra, t[fbb] - t[fa]), t[fa]) - z[:, :2]
    g = np.einsum("nij,njk,nk->ni", Ra, Wxy, e)                               # R_a Wxy e
    res2 = scatter(np.where(binary[:, None], -g, g), g, on)
    v = np.abs(np.einsum("nij,njk,nk->ni", Ra, Wxy, z[:, :2]))
    scale2 = float(scatter(v, v, on).max())
    r1, r2 = float(np.abs(res1).max()), float(np.abs(res2).max())
    return dict(res1=r1, res2=r2, scale1=scale1, scale2=scale2, rel1=r1 / scale1 if scale1 > 0 else r1, rel2=r2 / scale2 if scale2 > 0 else r2)


def exact_measurements(states, fa, fb):
    """z of every factor at the given states: zhat = pa^-1 o pb for an xyt factor, the pose itself for a prior"""
    x = np.asarray(states, float); fa = np.asarray(fa, np.int64); fb = np.asarray(fb, np.int64)
    binary = fb >= 0
    pa, pb = x[fa], x[np.where(binary, fb, 0)]
    d = np.einsum("nji,nj->ni", _rot(pa[:, 2]), pb[:, :2] - pa[:, :2])
    z = np.concatenate([d, mod2pi(pb[:, 2] - pa[:, 2])[:, None]], axis=1)
    z[~binary] = pa[~binary]
    return z
