"""Every step of the incremental path against the exact solution of its linear system.  TEST INFRASTRUCTURE.

`IncExact(lib, oracle)` stands in for a SolverLib (like `_Recorder` in tests/test_gpu_marginals.py), so the scenario drivers --
harness.run_demo / run_tutorial and the growth drivers of tests/test_gpu_parity.py -- run on it unchanged.  Every graph it makes
checks every april_graph_cholesky / _inc call on it:

* a batch call, or an incremental call that fell back to a batch step (param.batch_time changed): the normal-equation residual
  of the step at the l_points it left (tests/support/normal_eq.py), relative to the terms of the right-hand side, < `batch_tol`;
* an incremental step: x = the exact solution of the incremental system (tests/test_refmodel.py) -- every xyt
  factor at its poses' l_point as recorded before the call, every prior at the STATE of its node in the call that added it
  (april_graph_xytpos.c:83-85), Tikhonov only on the poses present at the last batch step -- solved by the oracle.  The poses
  whose state the step changed must hold l_point + x, the poses whose delta_X it changed delta_X = x, both within `inc_tol`;
  and the poses written / visited must be those the restated reference bookkeeping (aprilsam_amd_refmodel_*, fed with that x)
  predicts.  A predicted pose whose state did not change must hold l_point + x as well (it may have held it already).

A written set that differs from the prediction is tolerated only when some visited pose's exact |x| lies within 1e-8 of a
relinearisation threshold (the bookkeeping could then legitimately go either way); such steps are counted and logged.

`after_call(k, graph, written)` (optional) runs after the library call and before the check: the negative controls of
tests/test_inc_exact.py offset returned states there (host arithmetic on node objects, nothing on a device).
With strict=False nothing is asserted and the figures are only collected (`report`)."""
import ctypes as C

import numpy as np

from tests.support.normal_eq import mod2pi, normal_equation_residual

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
NEAR_THRESHOLD = 1e-8


def _i(a):
    return a.ctypes.data_as(_ip)


def _bind_model(dll):
    dll.aprilsam_amd_refmodel_create.restype = C.c_void_p
    dll.aprilsam_amd_refmodel_solve_visit.argtypes = [C.c_void_p, _dp, C.c_double, C.c_double, _ip]
    dll.aprilsam_amd_refmodel_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _ip]
    dll.aprilsam_amd_refmodel_inc_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _ip]
    dll.aprilsam_amd_refmodel_destroy.argtypes = [C.c_void_p]


def incremental_system(lp, fa, fb, z, W, q, n_batch, tikhanov):
    """The exact linear system of an incremental step, as the arguments Oracle.solve_system(lp, lp, fa, fb, zz, W, lam) takes:
    every xyt factor at its poses' l_point, every prior at q[i] -- the state of its node in the call that added it -- which gives the same rows
    as a prior at the l_point with z' = z - q + l_point; Tikhonov only on the poses present at the last batch step.  q: [F, 3], rows of binary
    factors unused.  -> (zz, lam)"""
    N = len(lp)
    zz = np.array(z, float)
    pr = np.nonzero(np.asarray(fb) < 0)[0]
    if len(pr):
        qq = np.asarray(q, float)[pr]; at = lp[np.asarray(fa)[pr]]
        moved = np.any(qq != at, axis=1)
        d = zz[pr] - qq; d[:, 2] = mod2pi(d[:, 2])
        zz[pr[moved]] = (d + at)[moved]
    return zz, np.where(np.arange(N) < n_batch, tikhanov, 0.0)


class IncExact:
    """lib stand-in: the graphs it makes check every solver call (module docstring).  stride: an incremental step that is not a
    fall-back, re-planned or low-rank-updated step is solved exactly only when its index (count of incremental calls so far on
    that graph) is a multiple of stride -- the others still feed the bookkeeping model, with the delta_X the library returned."""

    def __init__(self, lib, oracle, model_lib=None, inc_tol=1e-9, batch_tol=1e-10, stride=1, strict=True, after_call=None, log=None):
        self.lib, self.oracle = lib, oracle
        self.model = model_lib if model_lib is not None else lib
        _bind_model(self.model.dll)
        self.inc_tol, self.batch_tol, self.stride, self.strict = inc_tol, batch_tol, stride, strict
        self.after_call, self.log = after_call, log
        self.report = dict(inc_state=0.0, inc_delta=0.0, batch_res=0.0, batch=0, fallback=0, inc=0, checked=0, replanned=0,
                           updated=0, regen2=0, old_old=0, old_old_cross=0, near_threshold=0, failures=0, fallback_nodes=[], first_failure=None)

    def __getattr__(self, k):
        return getattr(self.lib, k)

    def set_option(self, name, value):
        if getattr(self.lib, "is_product", False):         # (the reference has no options: the drivers' set_option is a no-op there)
            self.lib.set_option(name, value)

    def new_graph(self):
        return _CheckedGraph(self, self.lib.new_graph())

    def summary(self):
        r = self.report
        return (f"inc |state - (lp + x)| {r['inc_state']:.2e}  |delta - x| {r['inc_delta']:.2e}  batch residual {r['batch_res']:.2e}  "
                f"steps: batch {r['batch']} fall-back {r['fallback']} (at {r['fallback_nodes']}) incremental {r['inc']} "
                f"(checked {r['checked']}, re-planned {r['replanned']}, low-rank updated {r['updated']}, >= 2 fronts regenerated "
                f"{r['regen2']}, with old-old factors {r['old_old']} of them cross-branch {r['old_old_cross']}) near-threshold {r['near_threshold']} failures {r['failures']}")

    def _fail(self, what):
        r = self.report
        r["failures"] += 1
        if r["first_failure"] is None:
            r["first_failure"] = what
        if self.strict:
            raise AssertionError(what)


class _CheckedGraph:
    def __init__(self, chk, g):
        self.chk, self.g = chk, g
        self.fa, self.fb, self.z, self.W, self.q = [], [], [], [], []       # factor cache; q: a prior's evaluation point
        self.M = None
        self.n_batch = 0
        self.n_inc = 0
        self.n_prev = 0                                   # poses at the previous solver call (a factor between two of them is old-old)

    def __getattr__(self, k):
        return getattr(self.g, k)

    def _sync_factors(self, st_now):
        g = self.g
        for i in range(len(self.fa), g.n_factors):
            f = g.factor(i)
            a = int(f.nodes[0]); b = int(f.nodes[1]) if f.nnodes == 2 else -1
            self.fa.append(a); self.fb.append(b)
            self.z.append([f.u.z[k] for k in range(3)]); self.W.append([f.u.W.contents.data[k] for k in range(9)])
            self.q.append(st_now[a].copy() if b < 0 else np.zeros(3))
        return np.array(self.fa, np.int32), np.array(self.fb, np.int32), np.array(self.z), np.array(self.W)

    def _batch_done(self, p, N, fa, fb, z, W, what):
        chk, r = self.chk, self.chk.report
        lp = self.g.l_points()
        res = normal_equation_residual(lp, fa, fb, z, W, self.g.deltas(), p.c.tikhanov)["rel_max"]
        r["batch_res"] = max(r["batch_res"], res)
        if not res < chk.batch_tol:
            chk._fail(f"{what} at {N} poses: normal-equation residual {res:.3e} >= {chk.batch_tol:.1e}")
        for i in range(len(self.q)):                      # a batch step evaluates every prior at the state it starts from (= l_point)
            if self.fb[i] < 0:
                self.q[i] = lp[self.fa[i]].copy()
        self.n_batch = N
        if self.M is None:
            self.M = C.c_void_p(chk.model.dll.aprilsam_amd_refmodel_create())
        chk.model.dll.aprilsam_amd_refmodel_batch(self.M, N, len(fa), _i(fa), _i(fb))

    def cholesky(self, p):
        st0 = self.g.states()
        fa, fb, z, W = self._sync_factors(st0)
        self.n_prev = len(st0)
        self.g.cholesky(p)
        if self.chk.after_call:
            self.chk.after_call(-1, self.g, None)
        self.chk.report["batch"] += 1
        self._batch_done(p, len(st0), fa, fb, z, W, "batch call")

    def cholesky_inc(self, p):
        chk, r, g = self.chk, self.chk.report, self.g
        st0, lp, d0 = g.states(), g.l_points(), g.deltas()
        N = len(st0)
        f0 = len(self.fa)
        fa, fb, z, W = self._sync_factors(st0)
        old_old = bool(np.any((fb[f0:] >= 0) & (np.maximum(fa[f0:], fb[f0:]) < self.n_prev)))
        self.n_prev = N
        bt = p.c.batch_time
        g.cholesky_inc(p)
        fell_back = p.c.batch_time != bt
        k = self.n_inc; self.n_inc += 1
        s = p.stats() if getattr(chk.lib, "is_product", False) else None
        if self.M is None:
            raise AssertionError("IncExact: an incremental call before any batch call on this graph")
        md = chk.model.dll
        md.aprilsam_amd_refmodel_inc_begin(self.M, N, len(fa), _i(fa), _i(fb))
        st1 = g.states()
        written = np.any(st1 != st0, axis=1)
        if chk.after_call:
            chk.after_call(k, g, written)
            st1 = g.states()
        d1 = g.deltas()
        if fell_back:
            r["fallback"] += 1; r["fallback_nodes"].append(N)
            x = np.ascontiguousarray(d1, float)           # (the model is rebuilt by the batch step right after)
            vis = np.zeros(N, np.int32)
            md.aprilsam_amd_refmodel_solve_visit(self.M, x.ctypes.data_as(_dp), p.c.delta_xy, p.c.delta_theta, _i(vis))
            self._batch_done(p, N, fa, fb, z, W, "fall-back")
            return
        r["inc"] += 1; r["old_old"] += old_old
        replanned = updated = False
        if s is not None:
            replanned = s["inc_replanned"] == 1; updated = s["inc_fronts_updated"] > 0
            r["replanned"] += replanned; r["updated"] += updated
            r["regen2"] += s["symbolic_reused"] == 1 and s["reserved0"] >= 2
            r["old_old_cross"] += s["inc_old_old_cross"] > 0
        check = replanned or updated or k % chk.stride == 0
        if check:
            zz, lam = incremental_system(lp, fa, fb, z, W, np.array(self.q, float).reshape(-1, 3), self.n_batch, p.c.tikhanov)
            x = np.ascontiguousarray(chk.oracle.solve_system(lp, lp, fa, fb, zz, W, lam))
        else:
            x = np.ascontiguousarray(d1, float)
        vis = np.zeros(N, np.int32)
        md.aprilsam_amd_refmodel_solve_visit(self.M, x.ctypes.data_as(_dp), p.c.delta_xy, p.c.delta_theta, _i(vis))
        if not check:
            return
        r["checked"] += 1
        upd, seen = vis == 2, vis > 0
        dchanged = np.any(d1 != d0, axis=1)
        e = st1 - (lp + x); e[:, 2] = mod2pi(e[:, 2])
        on = upd | written
        es = float(np.max(np.abs(e[on]), initial=0.0))
        on_v = seen | dchanged
        ed = float(np.max(np.abs(d1[on_v] - x[on_v]), initial=0.0))
        r["inc_state"] = max(r["inc_state"], es); r["inc_delta"] = max(r["inc_delta"], ed)
        form = f"step {k} ({N} poses{', re-planned' if replanned else ''}{', low-rank updated' if updated else ''})"
        if not (es <= chk.inc_tol and ed <= chk.inc_tol):
            worst = int(np.argmax(np.where(on[:, None], np.abs(e), 0).max(axis=1)))
            chk._fail(f"{form}: |state - (lp + x)| {es:.3e} (worst pose {worst}), |delta_X - x| {ed:.3e} > {chk.inc_tol:.0e}")
        extra_w, extra_v = written & ~upd, dchanged & ~seen
        if extra_w.any() or extra_v.any():
            ax = np.abs(x[seen | written | dchanged])
            near = ax.size and (np.min(np.abs(ax[:, :2] - p.c.delta_xy)) < NEAR_THRESHOLD or np.min(np.abs(ax[:, 2] - p.c.delta_theta)) < NEAR_THRESHOLD)
            if near:
                r["near_threshold"] += 1
                if chk.log:
                    chk.log(f"{form}: written / visited set differs from the model's next to a threshold (poses {np.nonzero(extra_w | extra_v)[0].tolist()})")
            else:
                chk._fail(f"{form}: poses written {np.nonzero(extra_w)[0].tolist()} / visited {np.nonzero(extra_v)[0].tolist()} "
                          f"that the reference bookkeeping does not touch")

    def destroy(self):
        if self.M is not None:
            self.chk.model.dll.aprilsam_amd_refmodel_destroy(self.M); self.M = None
        self.g.destroy()
