"""The contract of the retained factor, event by event and consumer by consumer.  TEST-ONLY.

include/aprilsam_amd.h says, entry point by entry point, which system "the LAST successful solver call on `param` factorised" is, which calls
drop the factor, which only end the audit's availability and which answer at the CURRENT states with the old Sigma.  This module crosses
the EVENTS that touch the graph, the param or the graph's device copy with the CONSUMERS that answer from what a solver call left behind:

    scene()        a 40-pose loop: an xytpos prior, odometry, three closures, full-matrix W, default tikhanov, started 5 cm / 0.02 rad off
                   so that a Gauss-Newton step moves the l_points by centimetres.  (No pose hangs off the loop by a single factor: such a
                   factor's post-fit residual is lambda-small and its chi2 no number a relative tolerance can hold; the event that
                   removes a leaf pose appends it first)
    System         a snapshot the TEST takes when a factorising call returns -- lp and Delta as the call left them, the factor arrays from
                   the test's own book-keeping (never read back from the library), lambda and the nodes that carry it -- with the dense A
                   and Sigma in float64
    CONSUMERS      each: the C call on sentinel-prefilled outputs, the project's existing checker against a System and the current host
                   states (tolerances unchanged: SIG_RTOL, GATE_RTOL and the 1e-7 rule of tests/test_gpu_consumer_paths.py, OMEGA_LIMIT,
                   audit_model.tolerances, ten times the float64 model's deviation from longdouble), and an "untouched" predicate
    EVENTS         functions of a Ctx (graph, param, the test's arrays, the Systems recorded so far)
    EXPECTED       event -> consumer -> the name of a System, or a return code, filled from the header (the line is cited beside each row)

judge() decides one cell from (return code, outputs, last error, fingerprints) alone, so tests/test_retained_contract_model.py can feed it
fabricated answers; shadow() restates the events that name a new System with numpy Gauss-Newton steps, so the same test can assert that the
replaced System's reference output FAILS every checker against the new one by a factor of 1000 (the discrimination condition)."""
import ctypes as C

import numpy as np

from tests.support import audit_model as am
from tests.support import marginal_prior_model as mm
from tests.support.gate_model import gate
from tests.support.normal_eq import mod2pi, normal_equation_residual
from tests.support.selinv_model import dense_system, system_blocks
from tests.support.sigma_compare import SIG_RTOL, check_any, check_blocks, random_pairs, ref_blocks, ref_joint, row_scale
from tests.support.treesolve_model import OMEGA_LIMIT, backward_error, relative_covariances, rhs_columns

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
GATE_RTOL = 1e-9                 # tests/test_gpu_gating.py, tests/test_gpu_consumer_paths.py
GATE_DENSE_RTOL = 1e-7           # the gate on the dense inverse's blocks: "1e-7 of every d2" (tests/test_gpu_consumer_paths._consumers)
NORMAL_EQ_RTOL = 1e-10           # the suite's bound on normal_equation_residual
SENT = -7.25                     # what every output holds before a call
LOOP = 40                        # poses of the loop
N0 = LOOP
TOP = LOOP - 2                   # every query names ids below 38: the nodes that every event's graph still holds (two are marginalised away)
CLOSURES = [(0, 39), (3, 30), (10, 25)]
DISCRIMINATION = 1000.0          # a replaced System's output must miss the new System's checker by this factor


def d_(a):
    return a.ctypes.data_as(_dp)


def i_(a):
    return a.ctypes.data_as(_ip)


# ---- scene ------------------------------------------------------------------------------------------------------------------------------
def _rel(pa, pb):
    c, s = np.cos(pa[2]), np.sin(pa[2])
    d = pb - pa
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], mod2pi(d[2])])


def scene(seed=5, n_loop=LOOP):
    """dict(start [N, 3], fa, fb, z [F, 3], W [F, 9]): factor 0 the xytpos prior on pose 0, then the odometry, then the closures.  Every W
    is a full symmetric positive definite matrix"""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n_loop) / n_loop
    truth = np.column_stack([5.0 * np.cos(a), 5.0 * np.sin(a), mod2pi(a + 0.5 * np.pi)])
    N = len(truth)
    start = truth + np.column_stack([rng.normal(0, 0.05, (N, 2)), rng.normal(0, 0.02, N)])

    def info():
        Q = rng.normal(size=(3, 3))
        W = Q @ Q.T * 4.0 + np.diag([100.0, 100.0, 400.0])
        return (0.5 * (W + W.T)).reshape(9)
    fa, fb, z, W = [0], [-1], [truth[0] + rng.normal(0, 0.01, 3)], [info()]
    closures = CLOSURES if n_loop == LOOP else [(0, n_loop - 1)]
    for x, y in [(i, i + 1) for i in range(N - 1)] + closures:
        fa.append(x); fb.append(y); W.append(info())
        z.append(_rel(truth[x], truth[y]) + [rng.normal(0, 0.02), rng.normal(0, 0.02), rng.normal(0, 0.01)])
    return dict(start=start, fa=np.array(fa, np.int32), fb=np.array(fb, np.int32), z=np.array(z, float), W=np.array(W, float))


def appended_pose(states, rng):
    """(state, z, W) of one more pose behind the graph's last node: odometry from that node, measured off the start by noise (the same W
    serves a closure from the new pose where an event adds one)"""
    last = np.asarray(states[-1], float)
    truth = last + [0.7 * np.cos(last[2]), 0.7 * np.sin(last[2]), 0.15]
    st = truth + np.r_[rng.normal(0, 0.05, 2), rng.normal(0, 0.02)]
    Q = rng.normal(size=(3, 3))
    W = Q @ Q.T * 4.0 + np.diag([100.0, 100.0, 400.0])
    return st, _rel(last, truth) + rng.normal(0, 0.01, 3), (0.5 * (W + W.T)).reshape(9)


# ---- System -----------------------------------------------------------------------------------------------------------------------------
class System:
    """the linear system of one factorising call: A = sum J'WJ + diag(lambda) at lp, Sigma = A^-1, and the step Delta it solved"""

    def __init__(self, name, lp, fa, fb, z, W, lam, lam_nodes=None, Delta=None, gauss=(), info=None, chi2_allow=None):
        self.name = name
        self.info = dict(info or {})               # families scene: the weight and the selection the effective slots were made with
        self.chi2_allow = chi2_allow               # [F] or None: what a polar factor's slot form costs its chi2 (audit_model.polar_chi2_allowance)
        self.lp = np.array(lp, float).reshape(-1, 3)
        self.fa, self.fb = np.array(fa, np.int32), np.array(fb, np.int32)
        self.z, self.W = np.array(z, float).reshape(-1, 3), np.array(W, float).reshape(-1, 9)
        self.lam, self.lam_nodes, self.gauss = float(lam), lam_nodes, list(gauss)
        self.N, self.Fg = len(self.lp), len(self.fa) + len(self.gauss)
        Aii, Aab = system_blocks(self.lp, self.fa, self.fb, self.z, self.W, self.lam, lam_nodes)
        self.A = dense_system(Aii, Aab, self.fa, self.fb)
        self.facs = am.xyt_factors(self.lp, self.fa, self.fb, self.z, self.W)
        self.B = am.dense_B(self.lp, self.facs)
        for nodes, xbar, eta, Lam in self.gauss:
            mm.gaussian_system(self.A, self.B, self.lp, nodes, xbar, eta, Lam)
        self.Sig = np.linalg.inv(self.A)
        self.scale = row_scale(self.Sig)
        self.ref = (self.Sig, self.scale)
        self.Delta = np.linalg.solve(self.A, self.B).reshape(-1, 3) if Delta is None else np.array(Delta, float).reshape(-1, 3)

    def sc(self):
        return dict(fa=self.fa, fb=self.fb, z=self.z, W=self.W.reshape(-1, 3, 3))


def gn_step(x, fa, fb, z, W, lam):
    """one Gauss-Newton step of the plain graph in numpy: (the System at x, the states after it)"""
    S = System("gn", x, fa, fb, z, W, lam)
    x1 = S.lp + S.Delta
    x1[:, 2] = mod2pi(x1[:, 2])
    return S, x1


# ---- consumers --------------------------------------------------------------------------------------------------------------------------
LIST = np.array([0, 7, 37, 20], np.int32)
ANY_A, ANY_B = (v.astype(np.int32) for v in random_pairs(TOP, 1, 30))            # both orders and a == b
ANCHOR = 7
REMOVE = np.array([20, 21], np.int32)                                            # the marginal-prior query: two adjacent poses
PRIOR_CAP = 8


def _gate_inputs():
    rng = np.random.default_rng(5)
    n, N = 20, TOP
    a = rng.integers(0, N, n).astype(np.int32); b = ((a + 1 + rng.integers(0, N - 1, n)) % N).astype(np.int32)
    z = rng.normal(size=(n, 3)) * [2, 2, 1]
    L = rng.normal(size=(n, 3, 3)) * 0.3 + np.eye(3) * 3
    return a, b, z, np.einsum("nij,nkj->nik", L, L).reshape(n, 9)


GATE_A, GATE_B, GATE_Z, GATE_W = _gate_inputs()
# marginals_joint: pairs of consecutive poses -- joined by a factor in every event's graph (odometry; after the marginalisation of 20 and
# 21 the renumbered pair (19, 20) by the Gaussian factor), so always on the pattern
BASE_PAIRS = (np.arange(TOP - 1, dtype=np.int32), np.arange(1, TOP, dtype=np.int32))


def _sent(*shape):
    return np.full(shape, SENT)


def _rel_err(got, ref, scale):
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(got, float) - ref)
    e = np.where(np.isnan(e), np.inf, e)
    return float(np.max(e / scale, initial=0.0))


class Consumer:
    """one entry point: call(lib, g, p, Nb) -> (rc, out) on sentinel-prefilled outputs, Nb the node count the caller believes the retained
    factor has; model(S, states) the reference output; ratio(out, S, states) the worst error over its tolerance (a pass is < 1);
    check(out, S, states) the project's checker, asserting; untouched(out)"""
    name = ""
    error_recorded = True          # a refusal sets aprilsam_amd_last_error
    discriminates = True           # its answer tells two systems of the same size apart
    success = staticmethod(lambda rc: rc == 0)

    def untouched(self, out):
        return all(bool(np.all(v == SENT)) for v in out.values())

    def blank(self, S, states):
        """the outputs as they are before a call (the shapes of model())"""
        return {k: np.full_like(v, SENT) for k, v in self.model(S, states).items()}

    tol = 1.0                      # what ratio() divides by (the default check reports ratio * tol: an error like the other checkers')

    def check(self, out, S, states):
        r = self.ratio(out, S, states)
        assert r < 1.0, (self.name, S.name, r)
        return r * self.tol


class MarginalsAll(Consumer):
    name = "marginals_all"

    def call(self, lib, g, p, Nb):
        cov = _sent(max(Nb, g.n_nodes) + 8, 3, 3)
        return lib.dll.aprilsam_amd_marginals(g.ptr, p.ptr, 0, None, d_(cov)), dict(cov=cov)

    def model(self, S, states):
        return dict(cov=ref_blocks(S.Sig, S.N, S.fa, S.fb)[0])

    def ratio(self, out, S, states):
        cov = out["cov"]
        if len(cov) < S.N or not np.all(cov[S.N:] == SENT):
            return np.inf
        return _rel_err(cov[:S.N].reshape(S.N, 9), ref_blocks(S.Sig, S.N, S.fa, S.fb)[0].reshape(S.N, 9), S.scale[:, None]) / SIG_RTOL

    def check(self, out, S, states):
        assert np.all(out["cov"][S.N:] == SENT)
        return check_blocks(S.ref, S.fa, S.fb, out["cov"][:S.N], ref_blocks(S.Sig, S.N, S.fa, S.fb)[1])


class MarginalsList(Consumer):
    name = "marginals_list"

    def call(self, lib, g, p, Nb):
        cov = _sent(len(LIST), 3, 3)
        return lib.dll.aprilsam_amd_marginals(g.ptr, p.ptr, len(LIST), i_(LIST), d_(cov)), dict(cov=cov)

    def model(self, S, states):
        return dict(cov=ref_blocks(S.Sig, S.N, S.fa, S.fb)[0][LIST])

    def ratio(self, out, S, states):
        return _rel_err(out["cov"].reshape(-1, 9), self.model(S, states)["cov"].reshape(-1, 9), S.scale[LIST][:, None]) / SIG_RTOL

    def check(self, out, S, states):
        d = ref_blocks(S.Sig, S.N, S.fa, S.fb)
        full = d[0].copy(); full[LIST] = out["cov"]                 # the listed blocks in their places, the dense inverse's elsewhere
        return check_blocks(S.ref, S.fa, S.fb, full, d[1])


class MarginalsJoint(Consumer):
    name = "marginals_joint"

    def call(self, lib, g, p, Nb):
        a, b = BASE_PAIRS
        cov = _sent(len(a), 6, 6)
        return lib.dll.aprilsam_amd_marginals_joint(g.ptr, p.ptr, len(a), i_(a), i_(b), d_(cov)), dict(cov=cov)

    def model(self, S, states):
        return dict(cov=ref_joint(S.Sig, *BASE_PAIRS))

    def ratio(self, out, S, states):
        a, b = BASE_PAIRS
        return _rel_err(out["cov"].reshape(-1, 36), ref_joint(S.Sig, a, b).reshape(-1, 36), np.maximum(S.scale[a], S.scale[b])[:, None]) / SIG_RTOL

    def check(self, out, S, states):
        return check_any(S.ref, *BASE_PAIRS, out["cov"])            # (every pair is joined by a factor: on the pattern, finite)


class JointAny(Consumer):
    name = "joint_any"

    def call(self, lib, g, p, Nb):
        cov = _sent(len(ANY_A), 6, 6)
        return lib.dll.aprilsam_amd_marginals_joint_any(g.ptr, p.ptr, len(ANY_A), i_(ANY_A), i_(ANY_B), d_(cov)), dict(cov=cov)

    def model(self, S, states):
        return dict(cov=ref_joint(S.Sig, ANY_A, ANY_B))

    def ratio(self, out, S, states):
        return _rel_err(out["cov"].reshape(-1, 36), ref_joint(S.Sig, ANY_A, ANY_B).reshape(-1, 36),
                        np.maximum(S.scale[ANY_A], S.scale[ANY_B])[:, None]) / SIG_RTOL

    def check(self, out, S, states):
        return check_any(S.ref, ANY_A, ANY_B, out["cov"])


class GateXyt(Consumer):
    """d2 and S of 20 candidates, and the joint blocks of the same pairs (a second call: what tests/test_gpu_consumer_paths._consumers
    feeds the model with)"""
    name = "gate_xyt"

    def call(self, lib, g, p, Nb):
        n = len(GATE_A)
        d2, S, J = _sent(n), _sent(n, 3, 3), _sent(n, 6, 6)
        rc = lib.dll.aprilsam_amd_gate_xyt(g.ptr, p.ptr, n, i_(GATE_A), i_(GATE_B), d_(GATE_Z), d_(GATE_W), d_(d2), d_(S))
        rc2 = lib.dll.aprilsam_amd_marginals_joint_any(g.ptr, p.ptr, n, i_(GATE_A), i_(GATE_B), d_(J))
        return (rc if rc == rc2 else ("gate_xyt", rc, "joint_any", rc2)), dict(d2=d2, S=S, joint=J)

    def model(self, S, states):
        J = ref_joint(S.Sig, GATE_A, GATE_B)
        d2, Sg = gate(states, GATE_A, GATE_B, GATE_Z, GATE_W, J)
        return dict(d2=d2, S=Sg, joint=J)

    def ratio(self, out, S, states):
        r = _rel_err(out["joint"].reshape(-1, 36), ref_joint(S.Sig, GATE_A, GATE_B).reshape(-1, 36),
                     np.maximum(S.scale[GATE_A], S.scale[GATE_B])[:, None]) / SIG_RTOL
        md2, mS = gate(states, GATE_A, GATE_B, GATE_Z, GATE_W, out["joint"])
        r = max(r, _rel_err(out["d2"], md2, np.abs(md2) + 1e-300) / GATE_RTOL, _rel_err(out["S"], mS, np.abs(mS).max()) / GATE_RTOL)
        md2b, _ = gate(states, GATE_A, GATE_B, GATE_Z, GATE_W, ref_joint(S.Sig, GATE_A, GATE_B))
        return max(r, _rel_err(out["d2"], md2b, np.abs(md2b)) / GATE_DENSE_RTOL)

    def check(self, out, S, states):
        worst = check_any(S.ref, GATE_A, GATE_B, out["joint"])
        md2, mS = gate(states, GATE_A, GATE_B, GATE_Z, GATE_W, out["joint"])
        d2 = out["d2"]
        assert np.abs(d2 - md2).max() < GATE_RTOL * np.abs(md2).max() and (np.abs(d2 - md2) <= GATE_RTOL * np.abs(md2) + 1e-300).all()
        assert np.abs(out["S"] - mS).max() < GATE_RTOL * np.abs(mS).max()
        md2b, _ = gate(states, GATE_A, GATE_B, GATE_Z, GATE_W, ref_joint(S.Sig, GATE_A, GATE_B))
        assert (np.abs(d2 - md2b) <= GATE_DENSE_RTOL * np.abs(md2b)).all()
        return max(worst, float((np.abs(d2 - md2b) / np.abs(md2b)).max()))


class Solve(Consumer):
    """FULL, FORWARD and BACKWARD applied to FORWARD's result, three right-hand sides (flat buffers with room behind the 9 N values)"""
    name = "solve"
    PAD = 72

    def call(self, lib, g, p, Nb):
        B = np.concatenate([np.ascontiguousarray(rhs_columns(Nb, 3, 11).T).ravel(), np.zeros(self.PAD)])
        X, Y, Z = (_sent(9 * Nb + self.PAD) for _ in range(3))
        f = lib.dll.aprilsam_amd_solve
        rc = [f(g.ptr, p.ptr, 0, 3, d_(B), d_(X)), f(g.ptr, p.ptr, 1, 3, d_(B), d_(Y))]
        rc.append(f(g.ptr, p.ptr, 2, 3, d_(Y if rc[1] == 0 else B), d_(Z)))
        return (rc[0] if rc[0] == rc[1] == rc[2] else tuple(rc)), dict(full=X, forward=Y, backward_of_forward=Z)

    def model(self, S, states):
        B = rhs_columns(S.N, 3, 11)
        L = np.linalg.cholesky(S.A)                                 # (any square root of A serves the reference: only FULL is compared)
        X = np.linalg.solve(S.A, B)
        pad = lambda v: np.concatenate([np.ascontiguousarray(v.T).ravel(), _sent(self.PAD)])
        return dict(full=pad(X), forward=pad(np.linalg.solve(L, B)), backward_of_forward=pad(X))

    def _full(self, out, S):
        X = np.asarray(out["full"]).ravel()
        if len(X) < 9 * S.N or not np.all(X[9 * S.N:] == SENT):
            return None
        return X[:9 * S.N].reshape(3, 3 * S.N).T

    def ratio(self, out, S, states):
        X = self._full(out, S)
        if X is None:
            return np.inf
        with np.errstate(invalid="ignore"):
            om = backward_error(S.A, X, rhs_columns(S.N, 3, 11))
        return float(np.max(np.where(np.isnan(om), np.inf, om))) / OMEGA_LIMIT

    def check(self, out, S, states):
        assert out["backward_of_forward"].tobytes() == out["full"].tobytes(), "FULL is not BACKWARD applied to FORWARD bit for bit"
        X = self._full(out, S)
        assert X is not None, "values written behind the 3 N entries of a vector"
        om = backward_error(S.A, X, rhs_columns(S.N, 3, 11))
        assert om.max() < OMEGA_LIMIT, om
        return float(om.max())


class Cross(Consumer):
    name = "marginals_cross"
    tol = SIG_RTOL

    def call(self, lib, g, p, Nb):
        cov = _sent(max(Nb, g.n_nodes) + 8, 3, 3)
        return lib.dll.aprilsam_amd_marginals_cross(g.ptr, p.ptr, ANCHOR, 0, None, d_(cov)), dict(cov=cov)

    def model(self, S, states):
        return dict(cov=S.Sig[:, 3 * ANCHOR:3 * ANCHOR + 3].reshape(S.N, 3, 3).copy())

    def ratio(self, out, S, states):
        cov = out["cov"]
        if len(cov) < S.N or not np.all(cov[S.N:] == SENT):
            return np.inf
        return _rel_err(cov[:S.N].reshape(S.N, 9), self.model(S, states)["cov"].reshape(S.N, 9),
                        np.maximum(S.scale, S.scale[ANCHOR])[:, None]) / SIG_RTOL


class Relative(Consumer):
    name = "relative_covariances"
    tol = GATE_RTOL

    def call(self, lib, g, p, Nb):
        cov = _sent(max(Nb, g.n_nodes) + 8, 3, 3)
        return lib.dll.aprilsam_amd_relative_covariances(g.ptr, p.ptr, ANCHOR, 0, None, d_(cov)), dict(cov=cov)

    def model(self, S, states):
        nodes = np.arange(S.N)
        Sii = ref_blocks(S.Sig, S.N, S.fa, S.fb)[0]
        Sia = S.Sig[:, 3 * ANCHOR:3 * ANCHOR + 3].reshape(S.N, 3, 3)
        return dict(cov=relative_covariances(states, ANCHOR, nodes, Sii[ANCHOR], Sii, Sia))

    def ratio(self, out, S, states):
        cov = out["cov"]
        if len(cov) < S.N or len(states) < S.N or not np.all(cov[S.N:] == SENT) or not np.all(cov[ANCHOR] == 0.0):
            return np.inf
        m = self.model(S, states)["cov"]
        others = np.arange(S.N) != ANCHOR
        return _rel_err(cov[:S.N][others].reshape(-1, 9), m[others].reshape(-1, 9), np.abs(m[others]).max(axis=(1, 2))[:, None]) / GATE_RTOL


class FactorisedNodes(Consumer):
    name = "factorised_nodes"
    error_recorded = False         # (-1 is its answer "none", not a failure: no device is asked, no error is recorded)
    discriminates = False          # (the node count: the same for a system and the one that replaced it)

    def call(self, lib, g, p, Nb):
        n = int(lib.dll.aprilsam_amd_factorised_nodes(p.ptr))
        return min(n, 0), dict(n=np.array([float(n)]))

    def model(self, S, states):
        return dict(n=np.array([float(S.N)]))

    def ratio(self, out, S, states):
        return 0.0 if out["n"][0] == S.N else np.inf

    def untouched(self, out):
        return out["n"][0] == -1

    def blank(self, S, states):
        return dict(n=np.array([-1.0]))


class FactorAudit(Consumer):
    name = "factor_audit"

    def success(self, rc):
        return not isinstance(rc, tuple) and rc >= 0               # (the count of factors that cannot be audited)

    def call(self, lib, g, p, Nb):
        rows = _sent(max(g.n_factors, 1) + 8, 4)
        return lib.dll.aprilsam_amd_factor_audit(g.ptr, p.ptr, 0, None, d_(rows)), dict(rows=rows)

    def model(self, S, states):
        rows = np.full((S.Fg, 4), np.nan)
        rows[:len(S.fa)] = am.audit(S.Sig, S.Delta, S.facs)          # (a dense Gaussian factor: four NaN, counted)
        return dict(rows=rows)

    def _parts(self, out, S):
        F = len(S.fa)
        got = out["rows"]
        ok = len(got) >= S.Fg and np.all(got[S.Fg:] == SENT) and np.isnan(got[F:S.Fg]).all()
        model = am.audit(S.Sig, S.Delta, S.facs)
        tol = am.tolerances(S.Sig, S.facs, model)
        if S.chi2_allow is not None:                # (zero for every factor but the polar ones)
            tol[:, 0] += np.asarray(S.chi2_allow)[:F] / np.maximum(np.abs(model[:, 0]), 1e-300)
        return ok, got[:F], model, tol

    def ratio(self, out, S, states):
        ok, got, model, tol = self._parts(out, S)
        if not ok or got.shape != model.shape:
            return np.inf
        with np.errstate(all="ignore"):
            r = [np.abs(got[:, 0] - model[:, 0]) / (tol[:, 0] * np.maximum(np.abs(model[:, 0]), 1e-300)), np.abs(got[:, 1] - model[:, 1]) / tol[:, 1],
                 np.abs(got[:, 3] - model[:, 3]) / tol[:, 3]]
        r = np.concatenate(r)
        return float(np.max(np.where(np.isnan(r), np.inf, r)))

    def check(self, out, S, states):
        ok, got, model, tol = self._parts(out, S)
        assert ok, "rows behind the factorised system written, or a Gaussian factor's row not NaN"
        worst, _ = am.compare(got, model, tol)
        return float(worst.max())


class MarginalPrior(Consumer):
    name = "marginal_prior"

    def call(self, lib, g, p, Nb):
        cap = PRIOR_CAP
        nk = C.c_int(-7); keep = np.full(cap, -7, np.int32)
        xbar, eta, L = _sent(3 * cap), _sent(3 * cap), _sent(9 * cap * cap)
        rc = lib.dll.aprilsam_amd_marginal_prior(g.ptr, p.ptr, len(REMOVE), i_(REMOVE), cap, C.byref(nk), i_(keep), d_(xbar), d_(eta), d_(L))
        return rc, dict(n_keep=np.array([float(nk.value)]), keep=keep.astype(float), xbar=xbar, eta=eta, Lambda=L)

    def untouched(self, out):
        return out["n_keep"][0] == -7 and np.all(out["keep"] == -7) and all(np.all(out[k] == SENT) for k in ("xbar", "eta", "Lambda"))

    def blank(self, S, states):
        out = Consumer.blank(self, S, states)
        out["n_keep"][:] = -7; out["keep"][:] = -7
        return out

    def _model(self, S, dtype):
        def extra(H, g):
            for nodes, xbar, eta, Lam in S.gauss:
                mm.gaussian_system(H, g, S.lp, nodes, xbar, eta, Lam)
        touching = [ga for ga in S.gauss if set(int(n) for n in ga[0]) & set(int(r) for r in REMOVE)]
        more = [n for ga in touching for n in ga[0]]
        return mm.marginal_prior(S.lp, S.fa, S.fb, S.z, S.W, REMOVE, dtype, extra if touching else None, more)

    def model(self, S, states):
        keep, xbar, eta, L = self._model(S, np.float64)
        nb = len(keep)
        out = dict(n_keep=np.array([float(nb)]), keep=np.full(PRIOR_CAP, -7.0), xbar=_sent(3 * PRIOR_CAP), eta=_sent(3 * PRIOR_CAP),
                   Lambda=_sent(9 * PRIOR_CAP * PRIOR_CAP))
        out["keep"][:nb] = keep; out["xbar"][:3 * nb] = xbar.ravel(); out["eta"][:3 * nb] = eta; out["Lambda"][:9 * nb * nb] = L.ravel()
        return out

    def ratio(self, out, S, states):
        """the rule of tests/test_gpu_marginal_prior._check: keep and xbar exact, Lambda symmetric bit for bit, eta and Lambda within ten
        times the float64 model's deviation from the longdouble model"""
        m64, ml = self._model(S, np.float64), self._model(S, np.longdouble)
        nb = len(ml[0])
        if int(out["n_keep"][0]) != nb or list(out["keep"][:nb].astype(int)) != list(ml[0]):
            return np.inf
        if not np.array_equal(out["xbar"][:3 * nb].reshape(nb, 3), S.lp[list(ml[0])]):
            return np.inf
        L = out["Lambda"][:9 * nb * nb].reshape(3 * nb, 3 * nb)
        if not np.array_equal(L, L.T):
            return np.inf
        r = 0.0
        for got, k in ((out["eta"][:3 * nb], 2), (L, 3)):
            allowed = 10 * float(np.max(np.abs(np.asarray(m64[k], np.longdouble) - ml[k])))
            err = float(np.max(np.abs(np.asarray(got, np.longdouble) - ml[k])))
            r = max(r, err / allowed if allowed > 0 else (0.0 if err == 0 else np.inf))
        return r


class Incremental(Consumer):
    """april_graph_cholesky_inc / _inc_solver are void and write into the graph: only the cells the header defines are in the table --
    "noop" (no factor: a silent return, states, l_points and delta_X keep their bits, no error recorded), -12 (a fixed node: refused, the
    code in aprilsam_amd_last_error, nothing written) and, for april_graph_cholesky_inc, "step": after a healthy batch call one appended
    pose takes a step that tests/support/inc_exact.IncExact accepts (run by the GPU test itself: it edits the graph)"""

    def __init__(self, name):
        self.name = name

    def call(self, lib, g, p, Nb):
        before = (g.states().tobytes(), g.l_points().tobytes(), g.deltas().tobytes())
        (g.cholesky_inc if self.name == "cholesky_inc" else g.cholesky_inc_solver)(p)
        after = (g.states().tobytes(), g.l_points().tobytes(), g.deltas().tobytes())
        code = lib.last_error()[0]
        return code, dict(same=np.array([SENT if before == after else 1.0]))


CONSUMERS = [MarginalsAll(), MarginalsList(), MarginalsJoint(), JointAny(), GateXyt(), Solve(), Cross(), Relative(), FactorAudit(),
             MarginalPrior(), FactorisedNodes(), Incremental("cholesky_inc"), Incremental("cholesky_inc_solver")]
BY_NAME = {c.name: c for c in CONSUMERS}
POOL = ["marginals_all", "marginals_list", "marginals_joint", "joint_any", "gate_xyt", "solve", "marginals_cross", "relative_covariances"]
LIN = ["factor_audit", "marginal_prior"]          # they read lp, Delta and the slots of the GRAPH's device copy
INC = ["cholesky_inc", "cholesky_inc_solver"]
ORDERS = {"forward": [c.name for c in CONSUMERS],
          # marginals before factor_audit before relative_covariances, and the reverse
          "audit_first": ["relative_covariances", "factor_audit", "marginals_all", "marginal_prior", "marginals_cross", "solve", "gate_xyt", "joint_any",
                          "marginals_joint", "marginals_list", "factorised_nodes", "cholesky_inc", "cholesky_inc_solver"]}


ORDERS["inc_first"] = INC + [n for n in ORDERS["forward"] if n not in INC]
ORDER_OF = {"02a_twice_forward": "forward", "02b_twice_audit_first": "audit_first", "22_node_fixed": "inc_first"}


# ---- the table --------------------------------------------------------------------------------------------------------------------------
def _row(pool, lin=None, n=None, inc="undefined", inc_solver=None, **over):
    """one event's row: `pool` for the consumers of the param's own pool, `lin` for the audit and the marginal prior (default: as pool),
    `n` for aprilsam_amd_factorised_nodes (default: as pool), then single cells"""
    row = {c: pool for c in POOL}
    row.update({c: (pool if lin is None else lin) for c in LIN})
    row["factorised_nodes"] = pool if n is None else n
    row["cholesky_inc"] = inc
    row["cholesky_inc_solver"] = inc if inc_solver is None and inc in ("noop", -12) else (inc_solver or "undefined")
    for k, v in over.items():
        assert k in row, k
        row[k] = v
    return row


# Values: the name of a System the event recorded ("S0" is what the two calls before every event leave); a return code of that entry point;
# for the two void incremental entry points "noop", -12, "step" (see Incremental) or "undefined" (the header defines no such cell: not run).
# Every row quotes the header (include/aprilsam_amd.h); tests/test_retained_contract_model.py checks that each quoted phrase stands there.
# h:NNN is the line it stood on when the row was written: a convenience, not a reference.
EXPECTED = {
    # h:447-453 "the system the LAST successful solver call on `param` factorised"; h:468-469 a second call only extracts
    "01_control": _row("S0", inc="step"),
    "02a_twice_forward": _row("S0", inc="step"),
    "02b_twice_audit_first": _row("S0", inc="step"),
    # h:453 "Sigma is recomputed in full after every solver call"
    "03_third_call": _row("S1", inc="step"),
    # h:496-499 / h:534-535 gate_xyt and relative_covariances: Jacobians at the CURRENT states, Sigma at the l_points of the last solver call;
    # h:854-857 the audit's lp and Delta live on the device: host states are not read
    "04_states_set": _row("S0", inc="step"),
    # h:857 "april_graph_chi2 alone does not"
    "05_chi2": _row("S0", inc="step"),
    # h:856-857 only "a factor's z / W edited and then evaluated by april_graph_chi2" ends the audit; h:474-475 (added): the edit alone is not seen
    "06_factor_edited": _row("S0", inc="undefined"),
    # h:856-857; h:764 the marginal prior is available exactly when the audit is
    "07_factor_edited_chi2": _row("S0", lin=-1),
    # h:850 "factors == NULL: all graph factors of the factorised system"; h:859 -13 only for a listed index outside them; h:474-475 (added)
    "08_factor_added": _row("S0"),
    # h:454 nodes == NULL: "the graph must hold exactly the factorised nodes" (-13, h:464); listed old nodes are in range; h:859-860 "a node
    # count that differs from the factorised one": -13; h:525-527 cross / relative: N <= the graph's nodes is enough
    "09_node_added": _row("S0", lin=-13, marginals_all=-13),
    # h:854-857 "another param's solver call on the graph -- a step, an LM or GNC run, a failed call -- ... ends the audit's availability";
    # the param's own pool is untouched (h:466-469); the incremental cell is out of scope
    "10_other_param_steps": _row("S0", lin=-1),
    "11_other_param_lm": _row("S0", lin=-1),
    "12_other_param_fails": _row("S0", lin=-1),
    # h:470-474 (added): the system is the PARAM's -- its last successful call was on ANOTHER graph of 25 nodes: ids of 25 and above are out
    # of range of the factorised system (h:464, h:502, h:525-527: -13); what takes no list answers for that system; h:853-854 "the param's
    # last call was made with another graph": -1
    "13_other_graph": _row(-13, lin=-1, n="SG2", marginals_cross="SG2", relative_covariances="SG2", solve="SG2"),
    # h:567-569 LM: "the retained factor DROPPED ... the next april_graph_cholesky_inc behaves as on a fresh param"; h:919 GNC; h:611-612 chordal
    "14_lm": _row(-1, inc="noop"),
    "15_gnc": _row(-1, inc="noop"),
    "16_chordal": _row(-1, inc="noop"),
    # h:456-457 "a resident run in progress", "also before its first step" (the second line added): -1; h:853 the audit too; h:460-461
    # (added): the incremental entry points "return silently, as on a param without a factorisation"
    "17_resident_open": _row(-1, inc="noop"),
    # h:457-459 (added): a loop that ended without a step leaves the factor that begin found, but begin took the graph's device copy (the
    # audit: -1, h:854-857) -- unless begin had to plan a changed graph: the fronts were laid out anew, the param is without a factor
    "17b_resident_unstepped": _row("S0", lin=-1),
    "17c_resident_replans_unstepped": _row(-1, inc="noop"),
    # h:428-430 "end leaves the node objects as the same number of april_graph_cholesky calls would ... the factorisation of that step is kept";
    # h:862-863 the audit is available after aprilsam_amd_resident_end and aprilsam_amd_batch_resident
    "18_resident_ended": _row("S_res", inc="step"),
    "19_batch_resident": _row("S_res", inc="step"),
    # h:269-273 after -2 the param's "FACTORISATION is dropped whatever it held before": the incremental entry points "return silently, the
    # covariance / gating / solve entry points return -1 and write nothing, aprilsam_amd_factorised_nodes returns -1"
    "20a_own_call_fails": _row(-1, inc="noop"),
    "20b_repaired": _row("S_new", inc="step"),
    # h:264-266 "For every code but -2 the param's cached plan and factorisation are dropped ... april_graph_cholesky_inc returns silently"
    "21_refused_minus_13": _row(-1, inc="noop"),
    # h:882-883 "a toggle after the factorisation drops the retained factor and they answer as without one"; h:884-887 marginals_cross and
    # relative_covariances refuse a graph with a fixed node with -12, april_graph_cholesky_inc and _inc_solver too while the param still
    # has its factor (they run first in this event: h:884-886, added).  aprilsam_amd_factorised_nodes takes no graph: -1 once a consumer
    # that does has seen the toggle (h:540-541, added)
    "22_node_fixed": _row(-1, inc=-12, marginals_cross=-12, relative_covariances=-12),
    # h:877 "fixing or freeing a node between two calls never re-plans"; the fixed set is the one the factor was made with again
    "23_fixed_and_freed": _row("S0", inc="step"),
    # h:449-453 after an incremental step lambda sits on the poses present at the last batch step; h:857-859 audit and prior: -12
    "24_inc_fast": _row("S_inc", lin=-12, inc="step"),
    # h:863 "an april_graph_cholesky_inc call that fell back to a batch step" makes the audit available
    "25_inc_fallback": _row("S_fb", inc="step"),
    # h:856 "an april_graph_cholesky_inc_solver call ... ends the audit's availability"; the factor is the one it solved with
    "26_inc_solver": _row("S0", lin=-1),
    # h:778 remove_nodes: "The graph's device copy is dropped" (the audit: -1, h:853-854); the param is not touched: its factor still has 41
    # nodes (S_leaf: the event's own call with the leaf), the graph 40 (marginals NULL: -13, h:454; relative_covariances: -13, h:525-527 "also of graph")
    "27_leaf_removed": _row("S_leaf", lin=-1, marginals_all=-13, relative_covariances=-13),
    # h:784-785 marginalize: "The param's plan and retained factor are dropped"
    "28a_marginalized": _row(-1, inc="noop"),
    # h:739-744 open to a graph with a Gaussian factor: solve, marginals, joint covariances, gating; the audit counts it (four NaN);
    # april_graph_cholesky_inc and _inc_solver refuse such a graph with -12
    "28b_reduced_solved": _row("S_red", inc=-12),
    # options are read when a call plans (h:286): nothing is dropped before one
    "29a_option_set": _row("S0", inc="step"),
    "29b_replanned": _row("S_new", inc="step"),
    # h:210 aprilsam_amd_param_set_device: "Whatever the param held (plan, fronts, captured graphs) is dropped"
    "30_slot_moved": _row(-1, inc="noop"),
    # h:470-474 (added): the param's pool is its own; the new graph has no device copy with this param's linearisation (h:853-854: -1)
    "31_graph_replaced": _row("S0", lin=-1),
}
CODES = {c: {-1, -12, -13} for c in POOL + LIN}
CODES["factorised_nodes"] = {-1}
CODES["cholesky_inc"] = {-12, "noop", "step", "undefined"}
CODES["cholesky_inc_solver"] = {-12, "noop", "undefined"}
SYSTEM_NAMES = {"S0", "S1", "SG2", "S_res", "S_new", "S_inc", "S_fb", "S_red", "S_leaf"}


def table_markdown(families=False):
    names = [c.name for c in CONSUMERS] + (FAM if families else [])
    lines = ["| event | " + " | ".join(names) + " |", "|---|" + "---|" * len(names)]
    for ev, row in (EXPECTED_FAM if families else EXPECTED).items():
        lines.append(f"| {ev} | " + " | ".join(str(row[n]) for n in names) + " |")
    return "\n".join(lines)


# ---- judging one cell -------------------------------------------------------------------------------------------------------------------
def judge(consumer, expected, rc, out, systems, states, err_code, fp_before, fp_after, replaced=None):
    """-> (complaints, worst): what is wrong with one cell's answer (an empty list: nothing), and the worst error over tolerance where a
    System was expected.  rc, out: what the call returned and left in the sentinel-prefilled outputs; err_code: aprilsam_amd_last_error
    after it (cleared before); fp_*: the fingerprints (plan fields of stats, selected inversions run, states, l_points, delta_X) around
    it; replaced: the System the expected one replaced -- the answer must NOT pass against it"""
    bad, worst = [], None
    if isinstance(expected, str) and expected in systems:
        S = systems[expected]
        if not consumer.discriminates:
            replaced = None
        if not consumer.success(rc):
            return [f"{consumer.name}: returned {rc} where the table says {expected}"], None
        try:
            worst = consumer.check(out, S, states)
        except AssertionError as e:
            bad.append(f"{consumer.name}: does not answer for {expected}: {str(e)[:200]}")
            if replaced is not None and consumer.ratio(out, replaced, states) < 1.0:
                bad.append(f"{consumer.name}: answers for the replaced system {replaced.name}")
        else:
            if replaced is not None and consumer.ratio(out, replaced, states) < 1.0:
                bad.append(f"{consumer.name}: passes against the replaced system {replaced.name} too: the scene does not discriminate")
    elif isinstance(expected, int):
        if rc != expected:
            bad.append(f"{consumer.name}: returned {rc} where the table says {expected}")
        if consumer.error_recorded and err_code != expected:
            bad.append(f"{consumer.name}: aprilsam_amd_last_error is {err_code}, not {expected}")
        if not consumer.untouched(out):
            bad.append(f"{consumer.name}: a refusal wrote into its outputs")
        if fp_before != fp_after:
            bad.append(f"{consumer.name}: a refusal changed {[k for k in fp_before if fp_before[k] != fp_after[k]]}")
    elif expected == "noop":
        if err_code != 0 or not consumer.untouched(out):
            bad.append(f"{consumer.name}: not a silent no-op (last error {err_code}, graph {'untouched' if consumer.untouched(out) else 'written'})")
        if fp_before != fp_after:
            bad.append(f"{consumer.name}: the no-op changed {[k for k in fp_before if fp_before[k] != fp_after[k]]}")
    else:
        raise ValueError((consumer.name, expected))
    return bad, worst


class DeviceTrouble(RuntimeError):
    """a HIP runtime call failed or a launch gave up waiting (-10 / -9): nothing more may run on this device in this process"""


# ---- the events on the library ----------------------------------------------------------------------------------------------------------
PLAN_FIELDS = ("n_nodes", "n_factors", "n_fronts", "n_levels", "max_front_rows", "nnz_L", "flops_factor", "bytes_fronts", "symbolic_reused")
NEG_W = np.diag([-1e6, -1e6, -1e6]).reshape(9)      # on the prior: the first pivot of pose 0 is negative (tests/test_gpu_not_spd.py's knob, coarser)


class Ctx:
    """graph, param and the test's own record of what the graph holds"""

    def __init__(self, lib, sc=None, opts=None):
        self.lib, self.opts = lib, dict(opts or {})
        sc = scene() if sc is None else sc
        self.fa, self.fb = list(sc["fa"]), list(sc["fb"])
        self.z, self.W = [np.array(v, float) for v in sc["z"]], [np.array(v, float) for v in sc["W"]]
        self.gauss = []
        self.g = self.build(sc["start"])
        self.p = lib.new_param()
        self.S, self.replaced, self.others = {}, {}, []
        self.rng = np.random.default_rng(77)
        self.cleanup = []                               # what has to happen before the closing call
        self.solvable = True

    def build(self, start):
        g = self.lib.new_graph()
        for s in start:
            g.add_node_xyt(s)
        for f in range(len(self.fa)):
            if self.fb[f] < 0:
                g.add_factor_xytpos(int(self.fa[f]), self.z[f], self.W[f])
            else:
                g.add_factor_xyt(int(self.fa[f]), int(self.fb[f]), self.z[f], self.W[f])
        return g

    def snapshot(self, name, lam_nodes=None, replaces=None):
        g, p = self.g, self.p
        self.S[name] = self.system(name, g.l_points(), lam_nodes, g.deltas())
        if replaces is not None:
            self.replaced[name] = self.S[replaces]
        return self.S[name]

    def system(self, name, lp, lam_nodes=None, Delta=None):
        return System(name, lp, self.fa, self.fb, self.z, self.W, self.p.c.tikhanov, lam_nodes, Delta=Delta, gauss=self.gauss)

    def ok(self, p=None):
        st = (p or self.p).stats()
        assert st["not_spd"] == 0 and st["error_code"] == 0, st

    def call(self, name=None, replaces=None):
        self.g.cholesky(self.p); self.ok()
        if name:
            self.snapshot(name, replaces=replaces)

    def start(self):
        """two successful calls: a captured graph exists, and they leave S0"""
        self.call(); self.call("S0")

    def edit(self, f, z=None, W=None):
        fac = self.g.factor(f)
        if z is not None:
            self.z[f] = np.array(z, float)
            for k in range(3):
                fac.u.z[k] = self.z[f][k]
        if W is not None:
            self.W[f] = np.array(W, float).reshape(9)
            for k in range(9):
                fac.u.W.contents.data[k] = self.W[f][k]

    def add_factor(self, a, b, z, W):
        self.g.add_factor_xyt(a, b, z, np.asarray(W).reshape(3, 3))
        self.fa.append(a); self.fb.append(b); self.z.append(np.array(z, float)); self.W.append(np.array(W, float).reshape(9))

    def add_pose(self, prior=False):
        """one more pose with its odometry; prior: and an xytpos prior on it (a leaf held by its odometry alone leaves the old poses'
        covariances exactly as they were: nothing could tell the extended system from the one before)"""
        st, z, W = appended_pose(self.g.states(), self.rng)
        n = self.g.add_node_xyt(st)
        self.add_factor(n - 1, n, z, W)
        if prior:
            zp = st + [0.02, -0.01, 0.005]
            self.g.add_factor_xytpos(n, zp, W.reshape(3, 3))
            self.fa.append(n); self.fb.append(-1); self.z.append(zp); self.W.append(W)
        return n

    def fingerprint(self):
        g, p = self.g, self.p
        try:
            st = p.stats()
            plan = tuple(st[k] for k in PLAN_FIELDS)
        except RuntimeError:
            plan = None
        return dict(plan=plan, selinv_runs=int(self.lib.dll.aprilsam_amd_debug_selinv_runs(p.ptr)), states=g.states().tobytes(),
                    l_points=g.l_points().tobytes(), delta_X=g.deltas().tobytes())

    def destroy(self):
        for o in self.others:
            o.destroy()
        self.p.destroy()
        if self.g is not None:
            self.g.destroy()


def _perturbed(ctx):
    x = ctx.g.states()
    return x + np.column_stack([ctx.rng.normal(0, 0.05, (len(x), 2)), ctx.rng.normal(0, 0.02, len(x))])


def _edit_closure(ctx):
    f = len(ctx.fa) - 1                                 # the closure (10, 25): z moved by decimetres, W doubled
    ctx.edit(f, z=ctx.z[f] + [0.3, -0.2, 0.05], W=2.0 * ctx.W[f])


def ev_control(ctx):
    pass


def ev_third_call(ctx):
    ctx.call("S1", replaces="S0")


def ev_states_set(ctx):
    ctx.g.set_all_states(_perturbed(ctx))


def ev_chi2(ctx):
    assert np.isfinite(ctx.g.chi2())


def ev_factor_edited(ctx):
    _edit_closure(ctx)


def ev_factor_edited_chi2(ctx):
    _edit_closure(ctx)
    assert np.isfinite(ctx.g.chi2())


def ev_factor_added(ctx):
    x = ctx.g.states()
    ctx.add_factor(5, 33, _rel(x[5], x[33]) + [0.05, -0.03, 0.01], ctx.W[3])


def ev_node_added(ctx):
    ctx.add_pose()


def _other_param(ctx):
    q = ctx.lib.new_param(); ctx.others.append(q)
    return q


def ev_other_param_steps(ctx):
    q = _other_param(ctx)
    ctx.g.set_all_states(_perturbed(ctx))               # (so that q's step moves the states by centimetres)
    ctx.g.cholesky(q); ctx.ok(q)


def ev_other_param_lm(ctx):
    q = _other_param(ctx)
    ctx.g.set_all_states(_perturbed(ctx))
    ctx.g.optimize_lm(q, max_iters=3)


def ev_other_param_fails(ctx):
    q = _other_param(ctx)
    W = ctx.W[0].copy()
    ctx.edit(0, W=NEG_W)
    ctx.g.cholesky(q)
    assert q.stats()["not_spd"] == 1 and ctx.lib.last_error()[0] == -2
    ctx.edit(0, W=W)


def ev_other_graph(ctx):
    sc2 = scene(seed=9, n_loop=25)
    c2 = Ctx.__new__(Ctx)
    c2.lib, c2.fa, c2.fb, c2.z, c2.W, c2.gauss = ctx.lib, list(sc2["fa"]), list(sc2["fb"]), list(sc2["z"]), list(sc2["W"]), []
    g2 = c2.build(sc2["start"]); ctx.others.append(g2)
    g2.cholesky(ctx.p); ctx.ok()
    ctx.S["SG2"] = System("SG2", g2.l_points(), c2.fa, c2.fb, c2.z, c2.W, ctx.p.c.tikhanov, Delta=g2.deltas())


def ev_lm(ctx):
    ctx.g.optimize_lm(ctx.p, max_iters=3)


def ev_gnc(ctx):
    cand = [f for f in range(len(ctx.fa)) if ctx.fb[f] >= 0 and abs(ctx.fa[f] - ctx.fb[f]) > 1]
    ctx.g.optimize_gnc(ctx.p, cand, max_stages=2, max_iters=3)


def ev_chordal(ctx):
    ctx.g.initialize_chordal(ctx.p)


def ev_resident_open(ctx):
    d = ctx.lib.dll
    assert d.aprilsam_amd_resident_begin(ctx.g.ptr, ctx.p.ptr) == 0
    ctx.cleanup.append(lambda: d.aprilsam_amd_resident_end(ctx.g.ptr, ctx.p.ptr))


def ev_resident_unstepped(ctx):
    d = ctx.lib.dll
    assert d.aprilsam_amd_resident_begin(ctx.g.ptr, ctx.p.ptr) == 0 and d.aprilsam_amd_resident_end(ctx.g.ptr, ctx.p.ptr) == 0


def ev_resident_replans_unstepped(ctx):
    """a factor added between two old poses: resident_begin plans the new graph, the loop ends without a step"""
    ev_factor_added(ctx)
    fronts = ctx.p.stats()["symbolic_reused"]
    ev_resident_unstepped(ctx)
    assert fronts == 1 and ctx.p.stats()["symbolic_reused"] == 0, "resident_begin was meant to plan anew"


def ev_resident_ended(ctx):
    d, g, p = ctx.lib.dll, ctx.g, ctx.p
    assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 2, 0) == 0
    assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
    assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    ctx.snapshot("S_res", replaces="S0")


def ev_batch_resident(ctx):
    ctx.g.batch_resident(ctx.p, 3)
    ctx.snapshot("S_res", replaces="S0")


def ev_own_call_fails(ctx):
    W = ctx.W[0].copy()
    ctx.edit(0, W=NEG_W)
    ctx.g.cholesky(ctx.p)
    assert ctx.p.stats()["not_spd"] == 1 and ctx.p.stats()["error_code"] == -2
    ctx.cleanup.append(lambda: ctx.edit(0, W=W))


def ev_repaired(ctx):
    ev_own_call_fails(ctx)
    ctx.cleanup.pop()()
    ctx.call("S_new", replaces="S0")


def ev_refused_minus_13(ctx):
    from aprilsam_amd import abi
    g = ctx.g
    g.add_factor_xyt(3, 3, [0, 0, 0], np.eye(3))
    g.cholesky(ctx.p)
    assert ctx.lib.last_error()[0] == -13 and ctx.p.stats()["error_code"] == -13
    fp = g.factor_ptr(g.n_factors - 1)
    g.ptr.contents.factors.contents.size -= 1           # the factor taken out again (the array's tail)
    abi.destroy_factor(fp)


def ev_node_fixed(ctx):
    assert ctx.g.set_fixed(12, True) == 0
    ctx.cleanup.append(lambda: ctx.g.set_fixed(12, False))


def ev_fixed_and_freed(ctx):
    assert ctx.g.set_fixed(12, True) == 0 and ctx.g.set_fixed(12, False) == 0


def ev_inc_fast(ctx):
    """two appended poses, a step each: a param's first incremental step plans anew to reserve the incremental path's slack (h:236-237:
    stats.inc_replanned), the second one extends that plan by a tail front"""
    n_batch = ctx.g.n_nodes
    bt = ctx.p.c.batch_time
    for _ in range(2):
        ctx.add_pose(prior=True)
        ctx.g.cholesky_inc(ctx.p); ctx.ok()
    st = ctx.p.stats()
    assert ctx.p.c.batch_time == bt, "the step was not meant to fall back to a batch step"
    assert st["inc_replanned"] == 0, "the second step was meant to take the fast path (under every option set this event runs with)"
    ctx.snapshot("S_inc", lam_nodes=n_batch, replaces="S0")


def ev_inc_fallback(ctx):
    ctx.add_pose(prior=True)
    bt = ctx.p.c.batch_time
    c = ctx.p.c                                         # every pose the walk visits counts as newly relinearised, and one is too many
    saved = (c.nthreshold, c.delta_xy, c.delta_theta)
    c.nthreshold, c.delta_xy, c.delta_theta = 0, 1e-12, 1e-12
    ctx.g.cholesky_inc(ctx.p); ctx.ok()
    c.nthreshold, c.delta_xy, c.delta_theta = saved
    assert ctx.p.c.batch_time != bt, "the step was meant to fall back to a batch step"
    ctx.snapshot("S_fb", replaces="S0")


def ev_inc_solver(ctx):
    ctx.g.cholesky_inc_solver(ctx.p)
    assert ctx.lib.last_error()[0] == 0


def ev_leaf_removed(ctx):
    """a pose appended behind the loop and solved with (S_leaf: 41 nodes), then taken out of the graph again"""
    leaf = ctx.add_pose()
    ctx.call("S_leaf", replaces="S0")
    idx = ctx.g.remove_nodes([leaf])
    assert idx[leaf] == -1 and ctx.g.n_nodes == leaf
    keep = [f for f in range(len(ctx.fa)) if leaf not in (ctx.fa[f], ctx.fb[f])]
    ctx.fa, ctx.fb, ctx.z, ctx.W = ([v[f] for f in keep] for v in (ctx.fa, ctx.fb, ctx.z, ctx.W))


def ev_marginalized(ctx):
    """the graph's states back at the l_points first, so that the prior is the exact marginal (h:760-761)"""
    g, p = ctx.g, ctx.p
    lp = g.l_points()
    g.set_all_states(lp)
    keep, xbar, eta, Lam = g.marginal_prior(p, REMOVE)
    fi, idx = g.marginalize(p, REMOVE)
    M = set(int(r) for r in REMOVE)
    left = [f for f in range(len(ctx.fa)) if ctx.fa[f] not in M and ctx.fb[f] not in M]
    ctx.fa = [int(idx[ctx.fa[f]]) for f in left]; ctx.fb = [int(idx[ctx.fb[f]]) if ctx.fb[f] >= 0 else -1 for f in left]
    ctx.z = [ctx.z[f] for f in left]; ctx.W = [ctx.W[f] for f in left]
    assert fi == g.n_factors - 1 == len(ctx.fa)
    # the Gaussian factor as the test's own model makes it from the scene at lp (never read back from the library)
    S0 = ctx.S["S0"]
    mk, mx, me, mL = mm.marginal_prior(lp, S0.fa, S0.fb, S0.z, S0.W, REMOVE, np.longdouble)
    assert list(mk) == list(keep)
    ctx.gauss = [([int(idx[b]) for b in mk], np.asarray(mx, float), np.asarray(me, float), np.asarray(mL, float))]


def ev_reduced_solved(ctx):
    ev_marginalized(ctx)
    ctx.call("S_red")


def ev_option_set(ctx):
    ctx.lib.set_option("leaf_nodes", 4)                 # (run_event restores the option)


def ev_replanned(ctx):
    ev_option_set(ctx)
    fronts = ctx.p.stats()["n_fronts"]
    ctx.call("S_new", replaces="S0")
    assert ctx.p.stats()["n_fronts"] != fronts and ctx.p.stats()["symbolic_reused"] == 0, "leaf_nodes was meant to force another tree"


def ev_slot_moved(ctx):
    assert ctx.lib.dll.aprilsam_amd_param_set_device(ctx.p.ptr, 3) == 0


def ev_graph_replaced(ctx):
    x = ctx.g.states()
    ctx.g.destroy()
    ctx.g = ctx.build(_perturbed_states(x, ctx.rng))


def _perturbed_states(x, rng):
    return x + np.column_stack([rng.normal(0, 0.05, (len(x), 2)), rng.normal(0, 0.02, len(x))])


EVENTS = {
    "01_control": ev_control, "02a_twice_forward": ev_control, "02b_twice_audit_first": ev_control, "03_third_call": ev_third_call,
    "04_states_set": ev_states_set, "05_chi2": ev_chi2, "06_factor_edited": ev_factor_edited, "07_factor_edited_chi2": ev_factor_edited_chi2,
    "08_factor_added": ev_factor_added, "09_node_added": ev_node_added, "10_other_param_steps": ev_other_param_steps,
    "11_other_param_lm": ev_other_param_lm, "12_other_param_fails": ev_other_param_fails, "13_other_graph": ev_other_graph, "14_lm": ev_lm,
    "15_gnc": ev_gnc, "16_chordal": ev_chordal, "17_resident_open": ev_resident_open, "17b_resident_unstepped": ev_resident_unstepped,
    "17c_resident_replans_unstepped": ev_resident_replans_unstepped, "18_resident_ended": ev_resident_ended,
    "19_batch_resident": ev_batch_resident, "20a_own_call_fails": ev_own_call_fails, "20b_repaired": ev_repaired,
    "21_refused_minus_13": ev_refused_minus_13, "22_node_fixed": ev_node_fixed, "23_fixed_and_freed": ev_fixed_and_freed,
    "24_inc_fast": ev_inc_fast, "25_inc_fallback": ev_inc_fallback, "26_inc_solver": ev_inc_solver, "27_leaf_removed": ev_leaf_removed,
    "28a_marginalized": ev_marginalized, "28b_reduced_solved": ev_reduced_solved, "29a_option_set": ev_option_set, "29b_replanned": ev_replanned,
    "30_slot_moved": ev_slot_moved, "31_graph_replaced": ev_graph_replaced,
}
TWICE = {"02a_twice_forward": "forward", "02b_twice_audit_first": "audit_first"}


def _new_id_refused(ctx):
    """a node added since the factorisation, asked for by its id: -13, nothing written (h:462)"""
    lib, nodes, cov = ctx.lib, np.array([ctx.g.n_nodes - 1], np.int32), _sent(1, 3, 3)
    lib.clear_error()
    rc = lib.dll.aprilsam_amd_marginals(ctx.g.ptr, ctx.p.ptr, 1, i_(nodes), d_(cov))
    ok = rc == -13 and lib.last_error()[0] == -13 and np.all(cov == SENT)
    return [] if ok else [f"marginals of the new node's id: returned {rc}, last error {lib.last_error()[0]}, outputs {'untouched' if np.all(cov == SENT) else 'written'}"]


EXTRA = {"09_node_added": _new_id_refused}       # cells outside the table's consumers


def run_event(lib, event, oracle=None, log=None, **opts):
    """the whole case under the options `opts`: two calls, the event, every consumer (judge), the closing call.  -> (complaints, record):
    record lists, per consumer, the return code and the bytes of every output, for the bitwise comparison of two runs.  Option
    "deterministic" is on: whether an incremental step falls back must not depend on the wall clock (h:287-290)"""
    with lib.options(deterministic=1, **opts):
        return _run_event(lib, event, oracle, log, opts)


def _run_event(lib, event, oracle, log, opts):
    ctx = (FamCtx if event in FAM_EVENTS else Ctx)(lib, opts=opts)
    bad, record, worst = [], [], {}
    leaf_nodes = lib.get_option("leaf_nodes")
    try:
        ctx.start()
        {**EVENTS, **FAM_EVENTS}[event](ctx)
        row = {**EXPECTED, **EXPECTED_FAM}[event]
        order = ORDERS[ORDER_OF.get(event, "forward")] if event in EVENTS else FAM_ORDER
        rounds = 2 if event in TWICE else 1
        runs0 = int(lib.dll.aprilsam_amd_debug_selinv_runs(ctx.p.ptr))
        for rnd in range(rounds):
            for name in order:
                if name not in row:
                    continue
                exp, cons = row[name], BY_NAME[name]
                if exp == "undefined" or (exp == "step" and (rnd < rounds - 1 or oracle is None)):
                    continue
                if exp == "step":
                    bad += _inc_step(ctx, oracle)
                    continue
                Nb = ctx.S[exp].N if isinstance(exp, str) and exp in ctx.S else ctx.g.n_nodes
                if name == "cholesky_inc":
                    # (it returns at once while the graph holds no factor the param has not seen, aprilsam.c:384-385, whatever else holds:
                    # the cell is run with one factor appended between two old poses)
                    x = ctx.g.states()
                    ctx.add_factor(6, 31, _rel(x[6], x[31]) + [0.05, -0.03, 0.01], ctx.W[3])
                lib.clear_error()
                fp0 = ctx.fingerprint()
                rc, out = cons.call(lib, ctx.g, ctx.p, Nb)
                err = lib.last_error()[0]
                if err in (-9, -10):
                    raise DeviceTrouble(f"{event}, {name}: {lib.last_error()}")
                fp1 = ctx.fingerprint()
                b, w = judge(cons, exp, rc, out, ctx.S, ctx.g.states(), err, fp0, fp1, ctx.replaced.get(exp) if isinstance(exp, str) else None)
                bad += b
                if w is not None:
                    worst[name] = max(worst.get(name, 0.0), w)
                record.append((name, rc, {k: v.tobytes() for k, v in out.items()}))
        if event in EXTRA:
            bad += EXTRA[event](ctx)
        if event in TWICE:                              # one Sigma pool and one selected inversion serve marginals, the audit and relative_covariances
            runs = int(lib.dll.aprilsam_amd_debug_selinv_runs(ctx.p.ptr)) - runs0
            if runs != 1:
                bad.append(f"{runs} selected inversions for one factorisation (two rounds of every consumer)")
        # a refusal must never cost the next call anything
        for undo in reversed(ctx.cleanup):
            undo()
        lib.set_option("leaf_nodes", leaf_nodes)
        if not ctx.gauss and not ctx.g.get_fixed(12):
            ctx.g.cholesky(ctx.p)
            st = ctx.p.stats()
            if st["not_spd"] or st["error_code"]:
                bad.append(f"the closing call failed: {st['error_code']} {lib.last_error()}")
            else:
                res = normal_equation_residual(ctx.g.l_points(), ctx.fa, ctx.fb, np.array(ctx.z), np.array(ctx.W), ctx.g.deltas(), ctx.p.c.tikhanov)["rel_max"]
                worst["closing_call_residual"] = res
                if not res < NORMAL_EQ_RTOL:
                    bad.append(f"the closing call's normal-equation residual is {res:.3e}")
                record.append(("closing", 0, dict(states=ctx.g.states().tobytes(), deltas=ctx.g.deltas().tobytes())))
        else:
            bad += _closing_gauss(ctx, worst, record)
        if log:
            log(f"[retained contract] {event}: worst error per consumer " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    finally:
        lib.set_option("leaf_nodes", leaf_nodes)
        ctx.destroy()
    return bad, record


def _closing_gauss(ctx, worst, record):
    """the closing call of a graph that holds the marginal prior as a Gaussian factor: against the dense model's step"""
    ctx.g.cholesky(ctx.p)
    st = ctx.p.stats()
    if st["not_spd"] or st["error_code"]:
        return [f"the closing call failed: {st['error_code']} {ctx.lib.last_error()}"]
    S = ctx.system("closing", ctx.g.l_points())
    res = float(np.max(np.abs(S.A @ ctx.g.deltas().reshape(-1) - S.B)) / np.max(np.abs(S.A) @ np.abs(ctx.g.deltas().reshape(-1)) + np.abs(S.B)))
    worst["closing_call_residual"] = res
    record.append(("closing", 0, dict(states=ctx.g.states().tobytes(), deltas=ctx.g.deltas().tobytes())))
    return [] if res < NORMAL_EQ_RTOL else [f"the closing call's residual is {res:.3e}"]


def _inc_step(ctx, oracle):
    """after a healthy batch call, one appended pose takes a step that IncExact accepts"""
    from tests.support.inc_exact import IncExact, _CheckedGraph
    chk = IncExact(ctx.lib, oracle)
    cg = _CheckedGraph(chk, ctx.g)
    try:
        cg.cholesky(ctx.p)
        ctx.add_pose()
        cg.cholesky_inc(ctx.p)
    except AssertionError as e:
        return [f"cholesky_inc: {str(e)[:300]}"]
    finally:
        if cg.M is not None:
            chk.model.dll.aprilsam_amd_refmodel_destroy(cg.M); cg.M = None
    return []



# ---- the families scene ------------------------------------------------------------------------------------------------------------------
# The same loop with one Cauchy closure, one two-component max-mixture closure, one range-bearing landmark (node 40) seen from two poses
# and one 2-node dense Gaussian factor away from the poses the marginal-prior query removes.  Its System is built from the EFFECTIVE slots of
# the numpy models at lp -- robust_model.weight, maxmix_model.select, the polar factor's xyt slot (polar_slot below: the header's formulas on
# polar_model's q, h and G), marginal_prior_model.gaussian_system -- without asking the device for w and sel.
from tests.support import maxmix_model as mxm          # noqa: E402
from tests.support import polar_model as pm            # noqa: E402
from tests.support import polar_gate_model as pgm      # noqa: E402
from tests.support import robust_model as rbm          # noqa: E402

LANDMARK = LOOP
ROBUST_PAIR, MAX_PAIR, POLAR_FROM, GAUSS_NODES = (5, 35), (8, 28), (12, 13), [30, 33]
WEIGHT_RTOL = 1e-12              # tests/test_gpu_robust.py's relative bound on what it computes from s = r'Wr


def polar_slot(kind, pa, pb, z, W):
    """(z_eff [3], W_eff [3, 3]) of include/aprilsam_amd.h: W_eff = [[G'WG, 0], [0, 0]], z_eff = (q + G'(GG')^-1 r, the predicted heading)"""
    q, _, _ = pm.rel(np.asarray(pa, float), np.asarray(pb, float))
    G = pm.G(kind, q)
    r = pm.residual(kind, z, q)
    m = pm.rows(kind)
    We = np.zeros((3, 3)); We[:2, :2] = G.T @ np.asarray(W, float).reshape(m, m) @ G
    ze = np.r_[q + G.T @ np.linalg.solve(G @ G.T, r), mod2pi(pb[2] - pa[2])]
    return ze, We


def families(seed=5):
    """the plain scene plus the family factors' definitions; the landmark's start is off its truth like every pose's"""
    sc = scene(seed)
    rng = np.random.default_rng(seed + 100)
    a = 2.0 * np.pi * np.arange(LOOP) / LOOP
    truth = np.column_stack([5.0 * np.cos(a), 5.0 * np.sin(a), mod2pi(a + 0.5 * np.pi)])
    lm = np.array([4.0, 5.2, 0.0])
    truth = np.vstack([truth, lm])
    W = np.diag([100.0, 100.0, 400.0])
    meas = lambda i, j, off=(0, 0, 0): _rel(truth[i], truth[j]) + rng.normal(0, 0.02, 3) * [1, 1, 0.5] + np.asarray(off, float)
    sc["start"] = np.vstack([sc["start"], lm + [0.05, -0.04, 0.0]])
    zm = meas(*MAX_PAIR)
    sc["fam"] = dict(
        robust=dict(a=ROBUST_PAIR[0], b=ROBUST_PAIR[1], z=meas(*ROBUST_PAIR, off=(0.15, -0.1, 0.03)), W=W.reshape(9), kind=rbm.CAUCHY, c=1.0),
        mix=dict(a=MAX_PAIR[0], b=MAX_PAIR[1], zs=np.array([zm, zm + [0.05, 0.02, 0.01]]), Ws=np.array([W.reshape(9), 0.1 * W.reshape(9)]), logw=np.array([mxm.LN09, mxm.LN01])),
        polars=[[pm.RANGE_BEARING, i, LANDMARK, pm.h(pm.RANGE_BEARING, pm.rel(truth[i], truth[LANDMARK])[0]) + rng.normal(0, 0.01, 2),
                 np.array([[2500.0, 30.0], [30.0, 10000.0]])] for i in POLAR_FROM])
    J = np.hstack([-np.eye(3), np.eye(3) + 0.1 * rng.normal(size=(3, 3))])
    Lam = J.T @ np.diag([50.0, 80.0, 300.0]) @ J
    Lam = 0.5 * (Lam + Lam.T)
    sc["fam"]["gauss"] = [GAUSS_NODES, truth[GAUSS_NODES] + rng.normal(0, 0.03, (2, 3)), Lam @ rng.normal(0, 0.05, 6), Lam]
    return sc


def fam_system(name, lp, plain, fam, lam, Delta=None):
    """the System of the families graph at lp from the effective slots"""
    lp = np.asarray(lp, float).reshape(-1, 3)
    fa, fb, z, W = (list(v) for v in plain)
    rb, mx = fam["robust"], fam["mix"]
    s_rb = float(rbm.s_of(lp, (np.array([rb["a"]]), np.array([rb["b"]]), np.array([rb["z"]]), np.array([rb["W"]])))[0])
    w = float(rbm.weight(rb["kind"], rb["c"], s_rb))
    fa.append(rb["a"]); fb.append(rb["b"]); z.append(rb["z"]); W.append(w * np.asarray(rb["W"]))
    sel = int(mxm.select(lp[mx["a"]], lp[mx["b"]], mx["zs"], mx["Ws"], mx["logw"]))
    fa.append(mx["a"]); fb.append(mx["b"]); z.append(mx["zs"][sel]); W.append(mx["Ws"][sel])
    allow = [0.0] * len(fa)
    for kind, i, j, zp, Wp in fam["polars"]:
        ze, We = polar_slot(kind, lp[i], lp[j], zp, Wp)
        fa.append(i); fb.append(j); z.append(ze); W.append(We.reshape(9))
        allow.append((ze, We))
    n_rb = len(plain[0])
    S = System(name, lp, fa, fb, z, W, lam, Delta=Delta, gauss=[tuple(fam["gauss"])], info=dict(w=w, sel=sel, rb=n_rb, mx=n_rb + 1))
    model = am.audit(S.Sig, S.Delta, S.facs)
    S.chi2_allow = np.array([am.polar_chi2_allowance(model[f, 0], *al) if isinstance(al, tuple) else 0.0 for f, al in enumerate(allow)])
    return S


class FamCtx(Ctx):
    def __init__(self, lib, opts=None):
        self.sc = families()
        self.fam = self.sc["fam"]
        Ctx.__init__(self, lib, self.sc, opts)
        self.gauss = [tuple(self.fam["gauss"])]

    def build(self, start):
        from aprilsam_amd import abi
        g = Ctx.build(self, start)
        rb, mx = self.fam["robust"], self.fam["mix"]
        g.add_factor_xyt(rb["a"], rb["b"], rb["z"], rb["W"])
        assert g.set_robust(g.n_factors - 1, rb["kind"], rb["c"]) == 0
        g.add_factor_max(mx["a"], mx["b"], mx["zs"], mx["Ws"], mx["logw"])
        for kind, i, j, zp, Wp in self.fam["polars"]:
            g.add_factor_polar(abi.POLAR_RANGE_BEARING, i, j, zp, Wp)
        g.add_factor_gaussian(*self.fam["gauss"])
        self.idx = dict(rb=len(self.fa), mx=len(self.fa) + 1, polar=len(self.fa) + 2, gauss=len(self.fa) + 4)
        return g

    def system(self, name, lp, lam_nodes=None, Delta=None):
        return fam_system(name, lp, (self.fa, self.fb, self.z, self.W), self.fam, self.p.c.tikhanov, Delta)


POLAR_CANDS = [(pm.RANGE_BEARING, 12, LANDMARK, [1.9, 0.4], [[2500.0, 30.0], [30.0, 10000.0]]), (pm.RANGE, 5, 20, [6.0], [[2500.0]]),
               (pm.BEARING, 30, 7, [0.3], [[10000.0]]), (pm.RANGE_BEARING, 14, LANDMARK, [2.4, -0.2], [[2500.0, 0.0], [0.0, 10000.0]])]
ASSOC_OBSERVER, ASSOC_LANDMARKS = 13, np.array([LANDMARK, 12, 25], np.int32)
ASSOC_OBS = [(pm.RANGE_BEARING, [1.6, 0.5], [[2500.0, 30.0], [30.0, 10000.0]]), (pm.RANGE, [3.0], [[2500.0]]), (pm.BEARING, [0.2], [[10000.0]])]


def _polar_arrays(cands):
    from aprilsam_amd.host import polar_candidates
    return polar_candidates([(k, z, W) for k, z, W in cands])


class GatePolar(Consumer):
    """d2 and S of four polar candidates and the joint blocks of their pairs (a second call, as GateXyt)"""
    name = "gate_polar"
    tol = GATE_RTOL

    def call(self, lib, g, p, Nb):
        n = len(POLAR_CANDS)
        a = np.array([c[1] for c in POLAR_CANDS], np.int32); b = np.array([c[2] for c in POLAR_CANDS], np.int32)
        kind, z, W = _polar_arrays([(c[0], c[3], c[4]) for c in POLAR_CANDS])
        d2, S, J = _sent(n), _sent(n, 2, 2), _sent(n, 6, 6)
        rc = lib.dll.aprilsam_amd_gate_polar(g.ptr, p.ptr, n, i_(a), i_(b), i_(kind), d_(z), d_(W), d_(d2), d_(S))
        rc2 = lib.dll.aprilsam_amd_marginals_joint_any(g.ptr, p.ptr, n, i_(a), i_(b), d_(J))
        return (rc if rc == rc2 else ("gate_polar", rc, "joint_any", rc2)), dict(d2=d2, S=S, joint=J)

    def _model(self, states, joint):
        a = [c[1] for c in POLAR_CANDS]; b = [c[2] for c in POLAR_CANDS]
        ok, d2, S = pgm.gate(states, a, b, [(c[0], np.array(c[3]), np.array(c[4])) for c in POLAR_CANDS], joint)
        assert ok.all()
        return d2, pgm.padded(S)

    def model(self, S, states):
        J = ref_joint(S.Sig, [c[1] for c in POLAR_CANDS], [c[2] for c in POLAR_CANDS])
        d2, Sg = self._model(states, J)
        return dict(d2=d2, S=Sg, joint=J)

    def ratio(self, out, S, states):
        a = np.array([c[1] for c in POLAR_CANDS]); b = np.array([c[2] for c in POLAR_CANDS])
        r = _rel_err(out["joint"].reshape(-1, 36), ref_joint(S.Sig, a, b).reshape(-1, 36), np.maximum(S.scale[a], S.scale[b])[:, None]) / SIG_RTOL
        if not np.isfinite(out["joint"]).all():
            return np.inf
        md2, mS = self._model(states, out["joint"])
        return max(r, _rel_err(out["d2"], md2, np.abs(md2) + 1e-300) / GATE_RTOL, _rel_err(out["S"], mS, np.abs(mS).max()) / GATE_RTOL)


class AssociatePolar(Consumer):
    """three observations from one pose against three nodes: the matrix, best, d2_best, d2_second; and the joint blocks of the pairs"""
    name = "associate_polar"
    tol = GATE_RTOL

    def call(self, lib, g, p, Nb):
        m, L = len(ASSOC_OBS), len(ASSOC_LANDMARKS)
        kind, z, W = _polar_arrays(ASSOC_OBS)
        d2, best, b1, b2, J = _sent(m, L), np.full(m, -7, np.int32), _sent(m), _sent(m), _sent(L, 6, 6)
        rc = lib.dll.aprilsam_amd_associate_polar(g.ptr, p.ptr, ASSOC_OBSERVER, m, i_(kind), d_(z), d_(W), L, i_(ASSOC_LANDMARKS), pgm.CHI2_1_999, pgm.CHI2_2_999,
                                                  d_(d2), i_(best), d_(b1), d_(b2))
        obs = np.full(L, ASSOC_OBSERVER, np.int32)
        rc2 = lib.dll.aprilsam_amd_marginals_joint_any(g.ptr, p.ptr, L, i_(obs), i_(ASSOC_LANDMARKS), d_(J))
        return (rc if rc == rc2 else ("associate_polar", rc, "joint_any", rc2)), dict(d2=d2, best=best.astype(float), d2_best=b1, d2_second=b2, joint=J)

    def untouched(self, out):
        return np.all(out["best"] == -7) and all(np.all(out[k] == SENT) for k in ("d2", "d2_best", "d2_second", "joint"))

    def blank(self, S, states):
        out = Consumer.blank(self, S, states)
        out["best"][:] = -7
        return out

    def _model(self, states, joint):
        return pgm.associate(states, ASSOC_OBSERVER, [(k, np.array(z), np.array(W)) for k, z, W in ASSOC_OBS], ASSOC_LANDMARKS, joint)

    def model(self, S, states):
        J = ref_joint(S.Sig, np.full(len(ASSOC_LANDMARKS), ASSOC_OBSERVER), ASSOC_LANDMARKS)
        m = self._model(states, J)
        return dict(d2=m["d2"], best=m["best"].astype(float), d2_best=m["d2_best"], d2_second=m["d2_second"], joint=J)

    def ratio(self, out, S, states):
        obs = np.full(len(ASSOC_LANDMARKS), ASSOC_OBSERVER)
        r = _rel_err(out["joint"].reshape(-1, 36), ref_joint(S.Sig, obs, ASSOC_LANDMARKS).reshape(-1, 36),
                     np.maximum(S.scale[obs], S.scale[ASSOC_LANDMARKS])[:, None]) / SIG_RTOL
        if not np.isfinite(out["joint"]).all():
            return np.inf
        m = self._model(states, out["joint"])
        if not np.array_equal(out["best"].astype(int), m["best"]):
            return np.inf
        for k in ("d2", "d2_best", "d2_second"):
            r = max(r, _rel_err(out[k], m[k], np.abs(m[k]) + 1e-300) / GATE_RTOL)
        return r


class RobustWeights(Consumer):
    """the weights of all factors: -1 for every factor but the Cauchy closure, whose weight is the numpy weight at the lp of the graph's most
    recent linearisation"""
    name = "robust_weights"
    tol = WEIGHT_RTOL

    def call(self, lib, g, p, Nb):
        n = g.n_factors
        idx = np.arange(n, dtype=np.int32); w = _sent(n + 4)
        return lib.dll.aprilsam_amd_robust_weights(g.ptr, p.ptr, n, i_(idx), d_(w)), dict(w=w)

    def model(self, S, states):
        w = _sent(S.Fg + 4); w[:S.Fg] = -1.0; w[S.info["rb"]] = S.info["w"]
        return dict(w=w)

    def ratio(self, out, S, states):
        m = self.model(S, states)["w"]
        got = out["w"]
        k = S.info["rb"]
        rest = np.arange(len(m)) != k
        if len(got) < len(m) or not np.array_equal(got[:len(m)][rest], m[rest]):
            return np.inf
        return abs(got[k] - m[k]) / abs(m[k]) / WEIGHT_RTOL


class MaxSelected(Consumer):
    name = "max_selected"
    discriminates = False          # (an index: two systems select the same component unless an edit flips it)

    def call(self, lib, g, p, Nb):
        n = g.n_factors
        idx = np.arange(n, dtype=np.int32); sel = np.full(n + 4, -7, np.int32)
        rc = lib.dll.aprilsam_amd_max_selected(g.ptr, p.ptr, n, i_(idx), i_(sel))
        return rc, dict(sel=sel.astype(float))

    def untouched(self, out):
        return np.all(out["sel"] == -7)

    def blank(self, S, states):
        return dict(sel=np.full(S.Fg + 4, -7.0))

    def model(self, S, states):
        sel = np.full(S.Fg + 4, -7.0); sel[:S.Fg] = -1; sel[S.info["mx"]] = S.info["sel"]
        return dict(sel=sel)

    def ratio(self, out, S, states):
        m = self.model(S, states)["sel"]
        return 0.0 if len(out["sel"]) >= len(m) and np.array_equal(out["sel"][:len(m)], m) else np.inf


FAM_ONLY = [GatePolar(), AssociatePolar(), RobustWeights(), MaxSelected()]
BY_NAME.update({c.name: c for c in FAM_ONLY})
FAM = [c.name for c in FAM_ONLY]
FAM_ORDER = [n for n in ORDERS["forward"] if n not in INC] + FAM + INC


def _fam_row(pool):
    """a families event's row: every consumer answers for `pool`; the graph holds a Gaussian factor, so the incremental entry points refuse"""
    row = _row(pool, inc=-12)
    row.update({c: pool for c in FAM})
    return row


def ev_robust_scale(ctx):
    ctx.fam["robust"]["c"] = 0.5
    assert ctx.g.set_robust(ctx.idx["rb"], ctx.fam["robust"]["kind"], 0.5) == 0


def ev_mixture_z(ctx):
    """the first component's z moved by metres: at the next linearisation the selection flips to the second component"""
    from aprilsam_amd import abi
    mx = ctx.fam["mix"]
    mx["zs"][0] = mx["zs"][0] + [3.0, -2.0, 0.5]
    comp = abi.max_view(ctx.g.factor(ctx.idx["mx"])).factors[0].contents
    for k in range(3):
        comp.u.z[k] = mx["zs"][0][k]


def ev_polar_z(ctx):
    pol = ctx.fam["polars"][0]
    pol[3] = pol[3] + [0.2, 0.05]
    f = ctx.g.factor(ctx.idx["polar"])
    for k in range(2):
        f.u.z[k] = pol[3][k]


def ev_gaussian_eta(ctx):
    ga = ctx.fam["gauss"]
    ga[2] = ga[2] + ga[3] @ np.array([0.1, -0.05, 0.02, 0.0, 0.08, -0.03])
    ctx.gauss = [tuple(ga)]
    f = ctx.g.factor(ctx.idx["gauss"])
    for k in range(6):
        f.u.z[6 + k] = ga[2][k]                         # (u.common.z: xbar, 3 k entries, then eta)


def _then_call(ev):
    def run(ctx):
        ev(ctx)
        ctx.call("S1", replaces="S0")
    return run


FAM_EDITS = {"32_robust_scale": ev_robust_scale, "33_mixture_z": ev_mixture_z, "34_polar_z": ev_polar_z, "35_gaussian_eta": ev_gaussian_eta}
FAM_EVENTS = {"F01_families_control": ev_control, **FAM_EDITS,
              **{"36" + "abcd"[i] + "_" + k[3:] + "_solved": _then_call(ev) for i, (k, ev) in enumerate(FAM_EDITS.items())}}
# robust losses (set_robust), max-mixture, polar and Gaussian factors in the header: "Wherever the solver linearises the factor" the scale, the
# selection, the slot and eta are read -- an edit in place changes nothing before the next linearisation, the consumers describe "the system
# that was factorised" (robust losses: "Marginals, joint covariances and gating describe the system that was factorised: the weighted one";
# aprilsam_amd_robust_weights / _max_selected: what "its most recent linearisation used"); the call after the edit factorises the edited system
EXPECTED_FAM = {ev: _fam_row("S1" if ev.startswith("36") else "S0") for ev in FAM_EVENTS}
FAM_NEW_SYSTEM_EVENTS = [ev for ev in FAM_EVENTS if ev.startswith("36")]
for _c in POOL + LIN + FAM:
    CODES.setdefault(_c, {-1, -12, -13})


def fam_shadow(event):
    """-> (S0, S1, states before, states after) of a families event that ends with a call: the edit applied to the numpy definitions, the
    Gauss-Newton steps taken on the effective systems"""
    sc = families()
    plain, fam, lam = (sc["fa"], sc["fb"], sc["z"], sc["W"]), sc["fam"], 1e-4

    def step(x, name):
        S = fam_system(name, x, plain, fam, lam)
        x1 = S.lp + S.Delta
        x1[:, 2] = mod2pi(x1[:, 2])
        return S, x1
    _, x1 = step(sc["start"], "gn")
    S0, x2 = step(x1, "S0")

    class _Defs:                                        # (what the edits touch of a FamCtx, without a library)
        pass
    d = _Defs(); d.fam = fam; d.gauss = None
    edit = FAM_EDITS[[k for k in FAM_EDITS if k[3:] in event][0]]
    if edit is ev_robust_scale:
        fam["robust"]["c"] = 0.5
    elif edit is ev_mixture_z:
        fam["mix"]["zs"][0] = fam["mix"]["zs"][0] + [3.0, -2.0, 0.5]
    elif edit is ev_polar_z:
        fam["polars"][0][3] = fam["polars"][0][3] + [0.2, 0.05]
    else:
        fam["gauss"][2] = fam["gauss"][2] + fam["gauss"][3] @ np.array([0.1, -0.05, 0.02, 0.0, 0.08, -0.03])
    S1, x3 = step(x2, "S1")
    return S0, S1, x2, x3


def fam_discrimination(event):
    old, new, x_old, x_new = fam_shadow(event)
    return {name: float(BY_NAME[name].ratio(BY_NAME[name].model(old, x_old), new, x_new)) for name in POOL + LIN + FAM}

# ---- the events in numpy: what the discrimination condition is asserted on ---------------------------------------------------------------
def shadow(event):
    """-> (old System, new System, old states, new states) of an event whose cells name a new System, or whose consumers read the states:
    the same scene and edits with numpy Gauss-Newton steps in place of the library's"""
    sc = scene()
    fa, fb, z, W = sc["fa"], sc["fb"], sc["z"], sc["W"]
    lam = 1e-4
    rng = np.random.default_rng(77)
    _, x1 = gn_step(sc["start"], fa, fb, z, W, lam)
    S0, x2 = gn_step(x1, fa, fb, z, W, lam)
    S0.name = "S0"
    if event in ("03_third_call", "20b_repaired", "29b_replanned"):
        S1, x3 = gn_step(x2, fa, fb, z, W, lam)
        return S0, S1, x2, x3
    if event in ("18_resident_ended", "19_batch_resident"):
        x = x2
        for _ in range(2 if event.startswith("18") else 3):
            S, x_next = gn_step(x, fa, fb, z, W, lam)
            x = x_next
        return S0, S, x2, x
    if event in ("04_states_set", "10_other_param_steps"):
        xp = _perturbed_states(x2, rng)
        if event.startswith("10"):
            _, xp = gn_step(xp, fa, fb, z, W, lam)
        return S0, S0, x2, xp
    if event == "27_leaf_removed":
        st, zz, WW = appended_pose(x2, rng)
        n = len(x2)
        S = System("S_leaf", np.vstack([x2, st]), np.r_[fa, n - 1], np.r_[fb, n], np.vstack([z, zz]), np.vstack([W, WW]), lam)
        return S0, S, x2, (S.lp + S.Delta)[:n]
    if event in ("24_inc_fast", "25_inc_fallback"):
        fast = event.startswith("24")
        n = len(x2)
        lp, nfa, nfb, nz, nW = (S0.lp if fast else x2), list(fa), list(fb), list(z), list(W)
        for k in range(2 if fast else 1):               # (an appended pose with its odometry and its prior, per step)
            st, zz, WW = appended_pose(np.vstack([x2, lp[n:]]), rng)
            nfa += [n + k - 1, n + k]; nfb += [n + k, -1]; nz += [zz, st + [0.02, -0.01, 0.005]]; nW += [WW, WW]
            lp = np.vstack([lp, st])
        S = System("S_inc", lp, nfa, nfb, np.array(nz), np.array(nW), lam, lam_nodes=n if fast else None)
        return S0, S, x2, lp + S.Delta
    if event == "28b_reduced_solved":
        lp = S0.lp
        mk, mx, me, mL = mm.marginal_prior(lp, fa, fb, z, W, REMOVE, np.longdouble)
        idx = np.full(len(lp), -1); keepn = [i for i in range(len(lp)) if i not in set(REMOVE.tolist())]; idx[keepn] = np.arange(len(keepn))
        left = [f for f in range(len(fa)) if fa[f] not in REMOVE and fb[f] not in REMOVE]
        gauss = [([int(idx[b]) for b in mk], np.asarray(mx, float), np.asarray(me, float), np.asarray(mL, float))]
        rfb = np.array([idx[fb[f]] if fb[f] >= 0 else -1 for f in left])
        S = System("S_red", lp[keepn], idx[fa[left]], rfb, z[left], W[left], lam, gauss=gauss)
        return S0, S, x2, lp[keepn] + S.Delta
    raise KeyError(event)


NEW_SYSTEM_EVENTS = ["03_third_call", "18_resident_ended", "19_batch_resident", "20b_repaired", "24_inc_fast", "25_inc_fallback", "27_leaf_removed",
                     "28b_reduced_solved", "29b_replanned"]
STATE_EVENTS = ["04_states_set", "10_other_param_steps"]


def discrimination(event):
    """{consumer: ratio}: the replaced System's reference output (at the OLD states) through the consumer's checker against the new System
    (at the new states).  inf where the output's very shape gives the old system away"""
    old, new, x_old, x_new = shadow(event)
    out = {}
    names = ["gate_xyt", "relative_covariances"] if event in STATE_EVENTS else [c for c in POOL + LIN + ["factorised_nodes"]]
    for name in names:
        cons = BY_NAME[name]
        if EXPECTED[event][name] not in SYSTEM_NAMES:
            continue
        try:
            ref = cons.model(old, x_old)
        except (IndexError, np.linalg.LinAlgError):
            continue
        try:
            out[name] = float(cons.ratio(ref, new, x_new))
        except (IndexError, ValueError):
            out[name] = np.inf                       # (the old system's output does not even have the new one's shape)
    return out
