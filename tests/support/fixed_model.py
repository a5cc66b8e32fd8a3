"""Fixed nodes, dense numpy.  TEST INFRASTRUCTURE: the restatement the GPU tests compare with.

With Phi the fixed set, a step solves the normal equations with the rows and columns of Phi removed.  The library keeps every node in
its place and masks instead: every block (i, j) with i or j in Phi zero, every right-hand-side segment of Phi zero, the diagonal block
of a node in Phi exactly 1.0 * I.  A and B come from the existing restatements (polar_model.system, which is lm_model.system plus the
polar factors); `mask` and `reduced_solve` are the two statements of the same step, and tests/test_fixed_model.py pins that they agree."""
import numpy as np

from tests.support import polar_model
from tests.support.normal_eq import mod2pi as _mod2pi

NO_POLARS = ()


def mod2pi(v):
    """the wrap the state update applies to every heading, as the kernel computes it: ((v + pi) - 2 pi floor((v + pi) / 2 pi)) - pi"""
    return _mod2pi(np.asarray(v, float))


def unchanged_by_wrap(v):
    """True where mod2pi returns v bitwise: the headings a fixed node keeps bitwise (not every v in [-pi, pi) is one)"""
    v = np.asarray(v, float)
    return mod2pi(v).view(np.uint64) == v.view(np.uint64)


def dofs(fixed):
    f = np.asarray(sorted(int(i) for i in fixed), np.int64)
    return (3 * f[:, None] + np.arange(3)[None, :]).ravel()


def system(x, plain, polars=NO_POLARS, lam=0.0):
    """dense (A, B) of the graph with nobody fixed: sum J'WJ + lam I and sum J'W r at x"""
    A, B = polar_model.system(np.asarray(x, float), plain, list(polars), lam)
    return np.asarray(A.todense()), np.asarray(B, float).copy()


def mask(A, B, fixed):
    """the system the library assembles: rows, columns and right-hand side of the fixed nodes zero, their diagonal exactly 1.0"""
    A = np.array(A, float, copy=True); B = np.array(B, float, copy=True)
    idx = dofs(fixed)
    A[idx, :] = 0.0; A[:, idx] = 0.0
    A[idx, idx] = 1.0
    B[idx] = 0.0
    return A, B


def reduced_solve(A, B, fixed, extra_diag=0.0):
    """d [3N]: (A_ff + extra_diag I) d_f = B_f on the free unknowns, zeros at the fixed ones"""
    n = len(B)
    free = np.setdiff1d(np.arange(n), dofs(fixed))
    d = np.zeros(n)
    Aff = np.asarray(A)[np.ix_(free, free)] + extra_diag * np.eye(len(free))
    d[free] = np.linalg.solve(Aff, np.asarray(B)[free])
    return d


def masked_solve(A, B, fixed):
    Am, Bm = mask(A, B, fixed)
    return np.linalg.solve(Am, Bm)


def step(x, d):
    """state = l_point + dx, every heading through mod2pi (fixed nodes included: their dx is 0)"""
    x1 = np.asarray(x, float) + np.asarray(d, float).reshape(-1, 3)
    x1[:, 2] = mod2pi(x1[:, 2])
    return x1


def conditional_covariance(A, fixed):
    """Sigma [3N, 3N] of the free nodes given the fixed ones: inv(A_ff) on the free unknowns, exact zeros in every row and column of a
    fixed node"""
    n = A.shape[0]
    free = np.setdiff1d(np.arange(n), dofs(fixed))
    S = np.zeros((n, n))
    S[np.ix_(free, free)] = np.linalg.inv(np.asarray(A)[np.ix_(free, free)])
    return S


# ---- the small graph of the tests: an 8-pose chain, two loop closures, an xytpos prior on node 5 ---------------------------------------
FIXED_SETS = [(0,), (3,), (0, 7), (2, 3), (5,)]


def _rel(pa, pb):
    c, s = np.cos(pa[2]), np.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, mod2pi(pb[2] - pa[2])])


def chain8(seed=3):
    """dict(start [8, 3], plain (fa, fb, z, W)): odometry 0-1-...-7, closures (0, 4) and (2, 7), a prior on node 5 (fb = -1).  Every
    start heading lies in [-pi, pi) and is returned bitwise by mod2pi (asserted): a fixed node then keeps all three components bitwise"""
    rng = np.random.default_rng(seed)
    truth = np.zeros((8, 3))
    for i in range(1, 8):
        t = truth[i - 1, 2]
        truth[i] = [truth[i - 1, 0] + np.cos(t), truth[i - 1, 1] + np.sin(t), mod2pi(t + 0.7)]
    pairs = [(i, i + 1) for i in range(7)] + [(0, 4), (2, 7)]
    fa, fb, z, W = [], [], [], []
    for a, b in pairs:
        fa.append(a); fb.append(b)
        z.append(_rel(truth[a], truth[b]) + rng.normal(0, [0.02, 0.02, 0.01]))
        M = rng.normal(0, 1, (3, 3))
        Wk = np.diag([400.0, 400.0, 2500.0]) + M @ M.T
        W.append((0.5 * (Wk + Wk.T)).reshape(9))
    fa.append(5); fb.append(-1); z.append(truth[5] + rng.normal(0, 0.01, 3)); W.append(np.diag([900.0, 900.0, 400.0]).reshape(9))
    start = truth + rng.normal(0, [0.05, 0.05, 0.03], truth.shape)
    start[:, 2] = mod2pi(start[:, 2])
    # headings the wrap returns bitwise: multiples of 2^-20, whose sum with the double pi is exact (checked, and nudged if it is not)
    start[:, 2] = np.round(start[:, 2] * 2.0 ** 20) / 2.0 ** 20
    for k in range(8):
        while not unchanged_by_wrap(start[k, 2]):
            start[k, 2] += 2.0 ** -20
    assert np.all(unchanged_by_wrap(start[:, 2])) and np.all(np.abs(start[:, 2]) < np.pi)
    plain = (np.array(fa, np.int64), np.array(fb, np.int64), np.array(z).reshape(-1, 3), np.array(W).reshape(-1, 9))
    return dict(start=start, truth=truth, plain=plain)


def build(lib, states, plain, polars=NO_POLARS, fixed=()):
    """the graph with its fixed set applied through aprilsam_amd_node_set_fixed"""
    g = polar_model.build(lib, states, plain, list(polars))
    for i in fixed:
        assert g.set_fixed(int(i), True) == 0
    return g
