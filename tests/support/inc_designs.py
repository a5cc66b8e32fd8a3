"""Incremental steps whose dirty fronts are DESIGNED: scenarios on the clique trees of tests/support/clique_trees.py.  TEST-ONLY.

The base graph is an anchored clique tree, solved with one batch step.  The first incremental call on a param always re-plans (the plan of a
param that never saw an incremental call has no room to append to: exit 3 of inc_fast_step), so every scenario opens with a PRIMER call that
adds one pose by odometry from the last pose (a pose of the root cluster).  The plan that call makes is the scenario's frozen base: the clique
tree's fronts, plus the primer pose as a leaf front of its own (s = 3, u = 3) under the root (tests/test_inc_designs.py holds every scenario to
that on the library's own plan).  Every later call adds poses chained by odometry from the newest pose, and factors between chosen poses:

* a factor from a pose of a leaf cluster to a new pose enters at that leaf's front and travels up every ancestor -- each front on the path
  gains one block row (u grows by 3) -- then through the tail fronts up to the one that owns the new pose;
* a second factor from the same cluster to the same new pose leaves the structure alone: the fronts are updated in place;
* a factor to an OLDER tail pose, after a newer one is already in a front's structure, gives that front a row that is not its last (mid).

`Model` restates the host bookkeeping of inc_fast_step (structure rows, dirty sets, tail fronts, eligibility for the low-rank update, array
capacities) front by front; what it predicts per step is what the scenario DECLARES, and tests/test_gpu_inc_shapes.py holds the library's own
record of the step (aprilsam_amd_debug_inc_forms) to it, field by field.  CLASSES names every size at which front_update_body, tail_refactor
or the eligibility rules change form, from the constants of the headers and independently of the scenarios; every scenario lists the classes
it is there for, tests/test_inc_designs.py checks that every class has a scenario and that the model's rows of that scenario show it, the GPU
test checks the same on the export."""
import os
import re

import numpy as np

from tests.support import clique_trees as CT

ROOT = CT.ROOT
SEED = 11
DELTA_XY = DELTA_THETA = 0.05


def _constants():
    """the limits of the incremental path, read from the headers that define them"""
    csrc = os.path.join(ROOT, "aprilsam_amd", "csrc")
    kern = open(os.path.join(csrc, "kernels.hip.h")).read()
    opts = open(os.path.join(csrc, "solver.h")).read()
    out = {}
    for name in ("UPD_MAXF", "UPD_MAXC", "TAIL_MAXF", "TAILQ", "INL_PATCHES", "WCAP", "CAPQ"):
        m = re.search(r"\b%s = (\d+)\b" % name, kern)
        assert m, name
        out[name] = int(m.group(1))
    m = re.search(r"\bTAILK = TAILQ / (\d+)\b", kern)
    assert m
    out["TAILK"] = out["TAILQ"] // int(m.group(1))
    body = kern[kern.index("void front_update_body("):kern.index("__global__ void __launch_bounds__(NT) k_front_small(")]
    m = re.search(r"for \(int k0 = 0; k0 < ns; k0 \+= (\d+)\)", body)             # forward substitution: columns per block
    assert m
    out["FS_BLOCK"] = int(m.group(1))
    m = re.search(r"for \(int j0 = 0; j0 < ns; j0 \+= (\d+)\)", body)             # T scan: columns per chunk
    assert m
    out["SCAN"] = int(m.group(1))
    m = re.search(r"for \(int pass = 0; pass \* (\d+) < nu \+ 1; pass\+\+\)", body)   # update block: rows per pass
    assert m
    out["PASS"] = int(m.group(1))
    m = re.search(r"update_front_lds\(R, 3 \* nsb, __builtin_popcount\(msk\)\) <= \(size_t\)(\d+) \* 1024", open(os.path.join(csrc, "solver_inc.inc.h")).read())
    assert m
    out["UPD_LDS"] = int(m.group(1)) * 1024
    for name in ("small_lds_kb", "small_threads", "tail_poses", "inc_one_up", "inc_one_dn", "inc_one_threads", "persist_max_fronts"):
        m = re.search(r"\b%s = (\d+)\b" % name, opts)
        assert m, name
        out[name] = int(m.group(1))
    return out


K = _constants()
NTS = (256, 512, 1024)                 # workgroup sizes front_update_body is instantiated with (k_front_small, k_inc_one)


def waves_of(nt):
    return 16 if nt >= 1024 else 8 if nt >= 512 else 4


def wl_bytes(nw):
    return K["CAPQ"] * 24 + nw * K["WCAP"] * 8 + nw * 64 * 8


def small_front_lds(R, C, nw):
    return (R | 1) * C * 8 + wl_bytes(nw)


def panel_front_lds(R, ns, nw):
    return (R | 1) * ns * 8 + wl_bytes(nw)


def update_front_lds(R, ns, nact):
    return (ns * (R | 1) + 3 * nact * (R | 1) + 8 * ns + 3 * (ns | 1) + 16) * 8


def popcount(v):
    return bin(int(v)).count("1")


# ------------------------------------------------------------------------------------------------------
# shape classes of an UPDATED front (a row of the export with mode 1), from the constants.  r: dict(ns, nu, nu_o, nact, mask, n_ch, ch_cnu,
# inplace, mid, own) -- ns, nu, nu_o in scalar rows (3 per pose); own: [(unary, the old pose comes first)] of the front's own new factors
# ------------------------------------------------------------------------------------------------------
FS, SC_, PS = K["FS_BLOCK"], K["SCAN"], K["PASS"]
def _trip(nt, over):
    """the children's vectors against one trip of nt threads: 3 (3 cnu + 1) entries; the first trip uses the prefetched block map, later ones reload it"""
    if over:
        return lambda r: r["nt"] == nt and any(nt < 3 * (3 * c + 1) <= nt + 9 for c in r["ch_cnu"])
    return lambda r: r["nt"] == nt and any(nt - 9 < 3 * (3 * c + 1) <= nt for c in r["ch_cnu"])


ROW_CLASSES = {
    f"ns last below {FS}: one partial block of the forward substitution": lambda r: FS - 3 <= r["ns"] < FS,
    f"ns = {FS + 1}: a last block of 1 column": lambda r: r["ns"] == FS + 1,
    f"ns = {2 * FS - 1}: a last block of {FS - 1} columns": lambda r: r["ns"] == 2 * FS - 1,
    f"ns last at or below {SC_}: one chunk of the T scan": lambda r: SC_ - 3 < r["ns"] <= SC_,
    f"ns first above {SC_}: the scan's carry": lambda r: SC_ < r["ns"] <= SC_ + 3,
    f"ns above {2 * SC_}: two carries": lambda r: r["ns"] > 2 * SC_,
    "ns mod 4 = 0": lambda r: r["ns"] % 4 == 0,
    "ns mod 4 = 1": lambda r: r["ns"] % 4 == 1,
    "ns mod 4 = 2": lambda r: r["ns"] % 4 == 2,
    "ns mod 4 = 3": lambda r: r["ns"] % 4 == 3,
    f"nu + 1 at or below {PS}: one pass over the update block": lambda r: 0 < r["nu"] and r["nu"] + 1 <= PS,
    f"nu + 1 in {PS + 1} .. {PS + 3}: a second pass, nearly empty": lambda r: PS + 1 <= r["nu"] + 1 <= PS + 3,
    f"nu + 1 above {2 * PS}: a third pass": lambda r: r["nu"] + 1 > 2 * PS,
    "nu mod 4 = 0": lambda r: r["nu"] % 4 == 0,
    "nu mod 4 = 1": lambda r: r["nu"] % 4 == 1,
    "nu mod 4 = 2": lambda r: r["nu"] % 4 == 2,
    "nu mod 4 = 3": lambda r: r["nu"] % 4 == 3,
    "nu_o = 0 growing to 3: a root gains its first update rows": lambda r: r["nu_o"] == 0 and r["nu"] == 3,
    "nu_o = nu: updated in place": lambda r: r["nu_o"] == r["nu"] and r["inplace"] == 1,
    "nu_o < nu: a fresh array in the grown layout": lambda r: r["nu_o"] < r["nu"] and r["inplace"] == 0,
    "nact = 1": lambda r: r["nact"] == 1,
    "nact = 2": lambda r: r["nact"] == 2,
    "nact = 3": lambda r: r["nact"] == 3,
    f"nact = {K['UPD_MAXF']} (UPD_MAXF)": lambda r: r["nact"] == K["UPD_MAXF"],
    "a mask that is a strict subset of the step's slots and does not start at slot 0 (si differs from the slot number)":
        lambda r: r["nact"] < r["step_slots"] and r["mask"] % 2 == 0,
    "a mask that is a strict, NON-CONTIGUOUS subset of the step's slots (slots {0, 2}): an updated tail front above a second component":
        lambda r: r["nact"] < r["step_slots"] and "101" in bin(r["mask"]),
    "an updated tail front": lambda r: r["tail"],
    "a front that sees two slot ranges through two children": lambda r: r["n_ch"] == 2 and r["nact"] >= 2,
    "n_ch = 0": lambda r: r["n_ch"] == 0,
    "n_ch = 1": lambda r: r["n_ch"] == 1,
    "n_ch = 2": lambda r: r["n_ch"] == 2,
    f"n_ch = {K['UPD_MAXC']} (UPD_MAXC)": lambda r: r["n_ch"] == K["UPD_MAXC"],
    "an own unary factor (lb < 0)": lambda r: any(un for un, _ in r["own"]),
    "an own binary factor, the old pose first": lambda r: any(not un and first for un, first in r["own"]),
    "an own binary factor, the new pose first": lambda r: any(not un and not first for un, first in r["own"]),
    f"update_front_lds just inside {K['UPD_LDS'] // 1024} KiB": lambda r: K["UPD_LDS"] - 1024 < update_front_lds(r["ns"] + r["nu"] + 3, r["ns"], r["nact"]) <= K["UPD_LDS"],
}
for _nt in (256, 512, 1024):
    ROW_CLASSES[f"a child's vectors last within one trip of {_nt} threads"] = _trip(_nt, False)
    ROW_CLASSES[f"a child's vectors first over one trip of {_nt} threads: the block map is reloaded"] = _trip(_nt, True)
# the rows of a STEP: rows = all its dirty fronts (dicts as above plus mode, front, tail), S = the step's summary
STEP_CLASSES = {
    f"exactly {K['UPD_MAXF']} new factors through updates": lambda rows, S: S["slots"] == K["UPD_MAXF"] and all(r["mode"] == 1 for r in rows if not r["last_tail"]),
    f"{K['UPD_MAXF'] + 1} new factors: the front that owns the last one and every common ancestor re-assembled above updated children":
        lambda rows, S: S["slots"] == K["UPD_MAXF"] and any(r["mode"] == 0 and r["n_dirty_ch_upd"] > 0 and not r["tail"] for r in rows),
    f"{K['UPD_MAXC']} dirty children under one updated front": lambda rows, S: any(r["mode"] == 1 and r["n_ch"] == K["UPD_MAXC"] for r in rows),
    f"update_front_lds just outside {K['UPD_LDS'] // 1024} KiB: the front re-assembled above an updated child":
        lambda rows, S: any(r["lds_refused"] and r["lds_refused"] <= K["UPD_LDS"] + 2048 and r["mode"] == 0 and r["n_dirty_ch_upd"] > 0 for r in rows),
    f"a front re-assembled above an updated child whose update block took a third pass (nu + 1 above {2 * PS})":
        lambda rows, S: any(r["mode"] == 0 and r["ch_upd_nu_max"] + 1 > 2 * PS for r in rows),
    "a mid front: re-assembled, its children updated": lambda rows, S: any(r["mid"] == 1 and r["mode"] == 0 and r["n_dirty_ch_upd"] > 0 for r in rows),
    "a new factor whose W fails the pivot test: its front re-assembled, the fronts below it updated":
        lambda rows, S: any(r["bad_w"] and r["mode"] == 0 for r in rows) and any(r["mode"] == 1 for r in rows),
    "a new factor whose W is asymmetric (by one ulp): its front re-assembled, the fronts below it updated":
        lambda rows, S: any(r["asym_w"] and r["mode"] == 0 and r["n_dirty_ch_upd"] > 0 for r in rows),
    "a tail front brought to exactly TAIL_POSES own poses": lambda rows, S: any(r["last_tail"] and r["nsb"] == S["TP"] for r in rows),
    "the step that opens the next tail front": lambda rows, S: S["opened"] > 0 and S["n_tail"] >= 2,
    f"tail_refactor with {K['TAIL_MAXF']} new factors (TAIL_MAXF)": lambda rows, S: S["tail_fast"] and S["n_fac"] == K["TAIL_MAXF"],
    f"{K['TAIL_MAXF'] + 1} new factors among the recent poses: no tail_refactor": lambda rows, S: not S["tail_fast"] and S["n_fac"] == K["TAIL_MAXF"] + 1 and S["all_recent"],
    f"tail_refactor over a window of exactly {K['TAILK']} poses (TAILK)": lambda rows, S: S["tail_fast"] and S["window"] == K["TAILK"],
    f"a window of {K['TAILK'] + 1} poses: no tail_refactor": lambda rows, S: not S["tail_fast"] and S["window"] == K["TAILK"] + 1 and S["all_recent"],
    "tail_refactor with a prior on a recent pose": lambda rows, S: S["tail_fast"] and S["has_prior"],
    "tail_refactor with two factors on one pair": lambda rows, S: S["tail_fast"] and S["dup_pair"],
    "tail_poses = 8": lambda rows, S: S["TP"] == 8 and S["tail_fast"],
    "tail_poses at its default": lambda rows, S: S["TP"] == K["tail_poses"] and S["tail_fast"],
}
# what only the library's record can show (the path a step took): claimed by a scenario's step, checked on the GPU against the export
PATH_CLASSES = {
    "solve_here taken": "tail+solve",
    "solve_here refused: a visited pose outside the window": "tail+list",
    "a general step as one k_inc_one": "one",
    "a general step in multi-level launches": "multi",
    "a general step in per-level launches": "levels",
    "tail_refactor on the general path": "tail general",
}
CLASSES = list(ROW_CLASSES) + list(STEP_CLASSES) + list(PATH_CLASSES)
# Sizes the issue names that no scenario of this table reaches, and why (tests/test_inc_designs.py prints them; nothing is asserted of them):
NOT_REACHED = {
    f"{K['UPD_MAXC'] + 1} updated children under one front": "every updated child brings at least one slot of its own and a step has UPD_MAXF = UPD_MAXC slots: a fifth dirty child "
        "is re-assembled for want of a slot, and its parent with it, before the count of children is looked at",
}


# ------------------------------------------------------------------------------------------------------
# the host bookkeeping of inc_fast_step, restated
# ------------------------------------------------------------------------------------------------------
class Model:
    """P: PlanView of the primed base graph (Nb poses).  step(...) -> ("re-plan", exit) or (S, rows)"""

    def __init__(self, P, Nb, tail_poses=None, inc_update=1, inc_multi=1, small_threads=None):
        self.P, self.Nb, self.nF0 = P, Nb, P.nF
        self.TP = tail_poses or K["tail_poses"]
        self.upd_on = bool(inc_update) and bool(inc_multi)
        self.tail_on = bool(inc_multi)
        self.small_threads = small_threads or K["small_threads"]
        self.nw = waves_of(self.small_threads)
        nF = P.nF
        self.nsb = [int(v) for v in P.front_nsb]
        self.nub0 = [int(v) for v in P.front_nub]
        self.parent = [int(v) for v in P.front_parent]
        self.base_parent = list(self.parent)
        self.pos_front = np.zeros(Nb, np.int64)
        for t in range(nF):
            self.pos_front[int(P.front_first[t]):int(P.front_first[t]) + self.nsb[t]] = t
        self.E = [[] for _ in range(nF)]
        self.cur_nub = list(self.nub0)
        self.cur_cap = [(3 * (self.nsb[t] + self.nub0[t] + 1)) * (3 * (self.nsb[t] + self.nub0[t])) for t in range(nF)]
        self.dirty = [0] * nF
        self.kids = [[] for _ in range(nF)]
        self.t_first, self.t_cnt, self.tf_of = [], [], []
        self.tail_ok, self.recs_stale = -1, -1
        self.N = Nb

    def front_of(self, node):
        return self.tf_of[node - self.Nb] if node >= self.Nb else int(self.pos_front[int(self.P.pos[node])])

    def children(self, t):
        if t >= self.nF0:
            return list(self.kids[t])
        return [int(c) for c in self.P.ch_idx[int(self.P.ch_ptr[t]):int(self.P.ch_ptr[t + 1])]]

    def _nsb(self, t):
        return self.t_cnt[t - self.nF0] if t >= self.nF0 else self.nsb[t]

    def _nub0(self, t):
        return 0 if t >= self.nF0 else self.nub0[t]

    def _owns(self, t, k):
        return t >= self.nF0 and self.t_first[t - self.nF0] <= k < self.t_first[t - self.nF0] + self.t_cnt[t - self.nF0]

    def _set_parent(self, t, par):
        if self.parent[t] == par:
            return
        if self.parent[t] >= self.nF0:
            self.kids[self.parent[t]].remove(t)
        self.parent[t] = par
        if par >= self.nF0:
            self.kids[par] = sorted(self.kids[par] + [t])

    def step(self, n_new, factors):
        """factors: [(a, b or -1, W ok for an update)] with node ids, in the order they are added"""
        nF0, Nb, TP = self.nF0, self.Nb, self.TP
        Nold, N = self.N, self.N + n_new
        fac = [(int(a), int(b)) for a, b, _ in factors]
        S = dict(TP=TP, n_fac=len(fac), tail_fast=False, window=None, opened=0, has_prior=any(b < 0 for a, b in fac),
                 dup_pair=len({(min(a, b), max(a, b)) for a, b in fac if b >= 0}) < sum(1 for a, b in fac if b >= 0), all_recent=False, slots=0)
        # ---- tail_refactor?
        tail_fast = False
        if self.t_first:
            first, n_old = self.t_first[-1], self.t_cnt[-1]
            n_fin = n_old + n_new
            lo = first + n_old
            S["all_recent"] = all(a >= first and (b < 0 or b >= first) for a, b in fac)
            for a, b in fac:
                lo = min(lo, min(a, b) if b >= 0 else a)
            if S["all_recent"]:
                S["window"] = n_fin - (lo - first)
            if self.tail_on and self.tail_ok == nF0 + len(self.t_first) - 1 and fac:
                ok = n_fin <= TP and not self.E[-1] and len(fac) <= K["TAIL_MAXF"] and S["all_recent"]
                if ok and n_fin - (lo - first) <= K["TAILK"]:
                    tail_fast = True
        S["tail_fast"] = tail_fast
        if not tail_fast and self.recs_stale >= 0:
            self.dirty[self.recs_stale] = 1
        # ---- 0. new poses
        grown_lo = 1 << 30
        for k in range(Nold, N):
            if not self.t_first or self.t_cnt[-1] >= TP:
                self.t_first.append(k); self.t_cnt.append(0)
                self.parent.append(-1); self.E.append([]); self.cur_nub.append(0); self.cur_cap.append(0); self.dirty.append(0); self.kids.append([])
                S["opened"] += 1
            self.t_cnt[-1] += 1
            t = nF0 + len(self.t_first) - 1
            self.tf_of.append(t); self.dirty[t] = 1
            grown_lo = min(grown_lo, t)
        self.N = N
        nFr = nF0 + len(self.t_first)
        S["n_tail"] = len(self.t_first)
        mid = [0] * nFr
        # ---- 1. owners, structure rows
        own = [[] for _ in range(nFr)]
        for i, (a, b) in enumerate(fac):
            ta, tb = a >= Nb, b >= Nb
            if b < 0:
                owner = self.front_of(a)
            elif ta != tb or (ta and tb):
                j, k = min(a, b), max(a, b)
                owner = self.front_of(j)
                t = owner
                while t >= 0 and not self._owns(t, k):
                    E = self.E[t]
                    if k not in E:
                        if E and E[-1] > k:
                            mid[t] = 1
                        E.append(k); E.sort(); self.dirty[t] = 1
                    if t >= nF0 or self.base_parent[t] < 0:
                        par = self.tf_of[E[0] - Nb]
                        if self.parent[t] >= 0 and self.parent[t] != par:
                            return ("re-plan", 6)
                        self._set_parent(t, par)
                    t = self.parent[t]
            else:
                raise NotImplementedError("factors between two base poses are not part of these scenarios")
            own[owner].append(i); self.dirty[owner] = 1
        for t in range(nFr):
            if self.dirty[t] and self.parent[t] >= 0:
                self.dirty[self.parent[t]] = 1
        # ---- 1b. eligibility
        small_max = K["small_lds_kb"] * 1024

        def dims(t):
            nsb = self._nsb(t)
            nub = self._nub0(t) + len(self.E[t])
            return nsb, nub

        def small(t, phantom):
            nsb, nub = dims(t)
            if phantom and t == nFr - 1 and not self.E[t]:
                nub += max(0, TP - nsb)
            R = 3 * (nsb + nub + 1)
            return small_front_lds(R, R - 3, self.nw) <= small_max or panel_front_lds(R, 3 * nsb, self.nw) <= small_max
        n_dirty = sum(self.dirty)
        all_small = all(small(t, True) for t in range(nFr) if self.dirty[t])
        if not all_small:
            return ("re-plan", 17)
        mode, fmask, n_slots = [0] * nFr, [0] * nFr, 0
        refused = [0] * nFr
        if self.upd_on and not tail_fast and n_dirty <= K["persist_max_fronts"]:
            for t in range(nFr):
                if not self.dirty[t] or t == nFr - 1 or t >= grown_lo or mid[t] or self.cur_cap[t] <= 0:
                    continue
                nsb, nub = dims(t)
                R = 3 * (nsb + nub + 1)
                ok = small(t, False)
                ndc, msk = 0, 0
                for ch in self.children(t):
                    if ok and self.dirty[ch]:
                        ok = mode[ch] != 0; msk |= fmask[ch]; ndc += 1
                ok = ok and ndc <= K["UPD_MAXC"]
                nown = 0
                for i in reversed(own[t]):
                    if not ok:
                        break
                    ok = factors[i][2] is True; nown += 1
                ok = ok and nown <= K["UPD_MAXF"] and n_slots + nown <= K["UPD_MAXF"]
                if ok:
                    for i in reversed(own[t]):
                        msk |= 1 << n_slots; n_slots += 1
                    ok = msk != 0 and update_front_lds(R, 3 * nsb, popcount(msk)) <= K["UPD_LDS"]
                    if msk != 0 and not ok:
                        refused[t] = update_front_lds(R, 3 * nsb, popcount(msk))
                if ok:
                    mode[t], fmask[t] = 1, msk
        S["slots"] = n_slots
        # ---- 2. the dirty fronts, children first
        rows = []
        for t in range(nFr):
            if not self.dirty[t]:
                continue
            tail = t >= nF0
            nsb, nub = dims(t)
            last_tail = tail and t == nFr - 1
            nph = max(0, TP - nsb) if (last_tail and not self.E[t]) else 0
            nub += nph
            nbc = nsb + nub
            need = (3 * (nbc + 1)) * (3 * nbc)
            old_nub = self.cur_nub[t]
            kids_d = [ch for ch in self.children(t) if self.dirty[ch]]
            r = dict(front=t, mode=mode[t], nsb=nsb, nub=nub, old_nub=old_nub, mask=fmask[t] if mode[t] else 0, n_own=len(own[t]) if mode[t] else 0,
                     n_ch=len(kids_d) if mode[t] else 0, mid=mid[t], ch_cnu=[self._nub0(ch) + len(self.E[ch]) for ch in kids_d] if mode[t] else [],
                     tail=tail, last_tail=last_tail, n_dirty_ch_upd=sum(1 for ch in kids_d if mode[ch]), bad_w=any(factors[i][2] is False for i in own[t]), asym_w=any(factors[i][2] == "asym" for i in own[t]),
                     own=[(fac[i][1] < 0, fac[i][0] < fac[i][1]) for i in own[t]] if mode[t] else [],
                     lds_refused=refused[t], ch_upd_nu_max=max([3 * (self._nub0(ch) + len(self.E[ch])) for ch in kids_d if mode[ch]], default=0), nt=self.small_threads, ns=3 * nsb, nu=3 * nub, nu_o=3 * old_nub, nact=popcount(fmask[t]) if mode[t] else 0, step_slots=n_slots)
            if tail_fast and last_tail:
                r["inplace"] = 1
                self.recs_stale = t
            else:
                if t == self.recs_stale:
                    self.recs_stale = -1
                fresh = (nub != old_nub) if mode[t] else need > self.cur_cap[t]
                if fresh:
                    gb = nbc if mode[t] else max(nbc + 4, TP + len(self.E[t]) + 4) if tail else nbc + 4
                    self.cur_cap[t] = (3 * (gb + 1)) * (3 * gb)
                r["inplace"] = 0 if fresh else 1
            self.cur_nub[t] = nub
            rows.append(r)
        if len(self.t_first) and self.dirty[nFr - 1]:
            self.tail_ok = nFr - 1
        for r in rows:
            self.dirty[r["front"]] = 0
        return S, rows


# ------------------------------------------------------------------------------------------------------
# scenarios.  A pose is ("c", cluster, k): pose k of base cluster `cluster` (clique_trees.layout order: leaves first, the root last), or
# ("n", j): the j-th pose added since the batch step (0 = the primer's); ("d", cluster, k): a pose of the second tree.  A step: dict(new = poses added (odometry from the newest pose, old
# pose first), fac = [(pose, pose or None for a prior, flags)]); flags: "", "semi" (a W of rank 2: fails the pivot test of the update) or
# "asym" (W[0][1] one ulp above W[1][0]: fails the symmetry test, and moves the exact system by 1e-16 of itself whichever triangle is taken)
# ------------------------------------------------------------------------------------------------------
def _c(cl, k=0):
    return ("c", cl, k)


def _n(j):
    return ("n", j)


SCENARIOS = {}


def _d(cl, k=0):
    return ("d", cl, k)


def _scenario(name, levels, fan, steps, claims, tail_poses=None, small_threads=None, second=None, why=""):
    """tail_poses, small_threads: options the scenario runs under, whatever the option set.  second: (levels, fan) of a second clique tree, not
    connected to the first, numbered behind it -- poses ("d", cluster, k); the primer's pose and the chain hang on the FIRST tree's last pose"""
    SCENARIOS[name] = dict(levels=tuple(levels), fan=fan, steps=steps, claims=claims, tail_poses=tail_poses, small_threads=small_threads, second=second, why=why)


# (6,5) x2: 17 poses -- the smallest tree with a leaf, a root and two children.  Clusters: 0, 1 leaves (6 poses, s = 18, u = 15), 2 root (5 poses, s = 15)
_scenario("6,5 x2: one leaf, then both", (6, 5), 2, [
    dict(new=1, fac=[(_c(0), _n(1), "")]),                                   # leaf 0 -> root -> tail; the primer's front too (odometry)
    dict(new=0, fac=[(_n(1), _c(0, 1), "")]),                                # the same leaf to the same pose, the new pose first: in place
    dict(new=1, fac=[(_c(0, 2), _n(2), ""), (_c(1), _n(2), "")]),            # both leaves: the root takes two children
    dict(new=0, fac=[(_c(0), None, ""), (_c(1, 3), _n(2), "")]),             # a prior on a leaf pose; in place
    dict(new=1, fac=[(_c(0, 4), _n(3), "")]),
], claims={1: ["a general step in multi-level launches", "nu_o = 0 growing to 3: a root gains its first update rows", "nact = 1", "n_ch = 0", "ns mod 4 = 2", "ns mod 4 = 3",
               "nu_o < nu: a fresh array in the grown layout", "an own binary factor, the old pose first", "nu mod 4 = 2", "nu mod 4 = 3",
               f"nu + 1 at or below {PS}: one pass over the update block"],
           2: ["nu_o = nu: updated in place", "an own binary factor, the new pose first", "n_ch = 1"],
           3: ["nact = 2", "n_ch = 2", "nu mod 4 = 1", "a front that sees two slot ranges through two children",
               "a mask that is a strict subset of the step's slots and does not start at slot 0 (si differs from the slot number)"],
           4: ["an own unary factor (lb < 0)"], 5: ["nu mod 4 = 0"]}, why="the smallest tree that has a leaf, a root and two children")

# ns on either side of 32 and 64: leaves of 11 / 22 poses over roots of 10 / 21
_scenario("11,10 x2: ns = 30 and 33", (11, 10), 2, [
    dict(new=1, fac=[(_c(0), _n(1), ""), (_c(1), _n(1), "")]),              # (the third slot: the odometry out of the primer's front)
    dict(new=1, fac=[(_c(0, 1), _n(2), "")]),
    dict(new=1, fac=[(_c(0, 2), _n(3), ""), (_c(1, 2), _n(3), ""), (_c(2), _n(3), "asym")]),      # the root owns a factor whose W is not symmetric to the bit
], claims={3: ["a new factor whose W is asymmetric (by one ulp): its front re-assembled, the fronts below it updated"],
           1: [f"ns last below {FS}: one partial block of the forward substitution", f"ns = {FS + 1}: a last block of 1 column", "ns mod 4 = 1", "nact = 3"]},
    why="ns = 30 (root) and 33 (leaves)")
_scenario("22,21 x2: ns = 63 and 66, nu + 1 = 67", (22, 21), 2, [
    dict(new=1, fac=[(_c(0), _n(1), ""), (_c(1), _n(1), "")]),
    dict(new=1, fac=[(_c(0, 1), _n(2), ""), (_c(0, 2), _n(2), ""), (_c(1, 1), _n(2), ""), (_c(2, 1), _n(2), "")]),
    dict(new=1, fac=[(_c(0, 1), _n(3), ""), (_c(0, 2), _n(3), ""), (_c(1, 1), _n(3), ""), (_c(1, 2), _n(3), ""), (_c(2, 1), _n(3), "")]),
], claims={1: [f"ns = {2 * FS - 1}: a last block of {FS - 1} columns", f"ns last at or below {SC_}: one chunk of the T scan", f"ns first above {SC_}: the scan's carry",
               f"nu + 1 in {PS + 1} .. {PS + 3}: a second pass, nearly empty", "nu mod 4 = 2"],
           2: [f"nact = {K['UPD_MAXF']} (UPD_MAXF)", f"exactly {K['UPD_MAXF']} new factors through updates"],
           3: [f"{K['UPD_MAXF'] + 1} new factors: the front that owns the last one and every common ancestor re-assembled above updated children"]},
    why="ns = 63 (root, one chunk of the scan, a last block of 31) and 66 (leaves, the carry); u = 63 + 3: a second 64-row pass of one row")
# ns mod 4 = 0: clusters of 8 poses (ns = 24); a W of rank 2 on a factor the root owns
_scenario("8,8 x2: ns = 24, a W that fails the pivot test", (8, 8), 2, [
    dict(new=1, fac=[(_c(0), _n(1), ""), (_c(1), _n(1), "")]),
    dict(new=1, fac=[(_c(0, 1), _n(2), ""), (_c(1, 1), _n(2), ""), (_c(2), _n(2), "semi")]),
], claims={1: ["ns mod 4 = 0"],
           2: ["a new factor whose W fails the pivot test: its front re-assembled, the fronts below it updated"]},
    why="ns = 24; a W of rank 2 on the root")
# the fan: 4 children under one front (UPD_MAXC), then a fifth dirty child (the primer's front, by odometry) -- "5 x4 deep, fan 4" gives the fan
_scenario("5 x3 deep, fan 4: UPD_MAXC children", (5, 5, 5), 4, [
    dict(new=1, fac=[]),                                                    # (the odometry alone: primer front -> root)
    dict(new=1, fac=[(_c(0), _n(2), ""), (_c(1), _n(2), ""), (_c(2), _n(2), ""), (_c(3), _n(2), "")]),      # the four leaves of middle front 16
    dict(new=1, fac=[(_c(0), _n(3), ""), (_c(16), _n(3), ""), (_c(4), _n(3), "")]),      # a leaf, its parent's own factor, a leaf of the next middle front
], claims={2: [f"n_ch = {K['UPD_MAXC']} (UPD_MAXC)", f"{K['UPD_MAXC']} dirty children under one updated front"]}, why="four leaves under one front")
# the children's vectors on either side of one trip of the workgroup: 3 (3 cnu + 1) entries against NT.  The fronts of a closure's path run in the
# multi-level launch at small_threads (k_inc_one takes steps that walk at most inc_one_dn fronts back down: a closure's walk is longer), so the
# scenario sets small_threads.  NT = 256: a leaf with 28, then 29 update blocks (255, 264).  NT = 512: 56, then 57 (507, 516)
_scenario("28,27 x2: a child's vectors around 256 threads", (28, 27), 2, [
    dict(new=1, fac=[]),
    dict(new=1, fac=[(_c(0), _n(2), "")]),
    dict(new=1, fac=[(_c(0, 1), _n(3), "")]),
    dict(new=1, fac=[(_c(0, 2), _n(4), ""), (_c(2), _n(4), "semi")]),         # (the root re-assembled above the leaf)
], claims={2: ["a child's vectors last within one trip of 256 threads"],
           3: ["a child's vectors first over one trip of 256 threads: the block map is reloaded"]}, small_threads=256,
    why="cnu = 28 and 29: the smallest tree whose leaf has 27 ancestor poses")
_scenario("20,19,19,17 x2: a child's vectors around 512 threads", (20, 19, 19, 17), 2, [
    dict(new=1, fac=[(_c(0), _n(1), "")]),
    dict(new=1, fac=[(_c(0, 1), _n(2), "")]),
    dict(new=1, fac=[(_c(0, 2), _n(3), ""), (_c(8), _n(3), "semi")]),         # (the leaf's parent re-assembled above it)
], claims={1: ["a child's vectors last within one trip of 512 threads"],
           2: ["a child's vectors first over one trip of 512 threads: the block map is reloaded"]}, small_threads=512,
    why="cnu = 56 and 57: leaves of 20 poses under 55 ancestor poses; 291 poses, the largest tree of the table")
# NT = 1024, the default of the multi-level launch: cnu = 113, then 114 (1 020, 1 029).  No clique tree within the size bound has a single-workgroup
# front with that many update rows in its base plan, so a small leaf gains them: one re-assembled call adds 107 poses, each closed to the leaf
# (tail fronts of 8 poses, so that every tail front on the way stays a single-workgroup front); the two calls behind it are updates again, through
# the leaf, the root and a chain of fourteen updated tail fronts
_scenario("6,5 x2: a leaf that gains 107 rows, a child's vectors around 1024 threads", (6, 5), 2, [
    dict(new=107, fac=[(_c(0, j % 6), _n(j), "") for j in range(1, 108)] + [(_n(j), None, "") for j in range(1, 108)]),      # (a prior on every new pose, as the base has: a chain of a hundred free poses costs the reference digits)
    dict(new=1, fac=[(_c(0), _n(108), ""), (_n(108), None, "")]),
    dict(new=1, fac=[(_c(0, 1), _n(109), ""), (_n(109), None, "")]),
    dict(new=1, fac=[(_c(0, 2), _n(110), ""), (_c(2), _n(110), "semi"), (_n(110), None, "")]),       # (the root re-assembled above the leaf)
], claims={2: ["a child's vectors last within one trip of 1024 threads"],
           3: ["a child's vectors first over one trip of 1024 threads: the block map is reloaded"]}, tail_poses=8,
    why="17 base poses and 111 added: rows gained through the structure, not through the base plan")
# ns above 128 and the LDS limit of the update: a root of 43 poses (ns = 129) is a single-workgroup front only with 256 threads; its leaves (s = 132,
# u = 129) are multi-workgroup fronts and stay clean -- the factors go to root poses and to the primer's pose
_scenario("44,43 x4: ns = 129 at the LDS limit", (44, 43), 4, [
    dict(new=1, fac=[(_c(4), _n(1), ""), (_c(4, 1), _n(1), ""), (_c(4, 2), _n(1), "")]),       # nu = 3, four slots: 163 760 bytes of 163 840
    dict(new=1, fac=[(_n(0), _n(2), ""), (_c(4), _n(2), ""), (_c(4, 1), _n(2), "")]),         # nu = 6, three slots: 164 936 bytes -- re-assembled above the primer's front
    dict(new=1, fac=[(_c(4), _n(3), "")]),                                                   # nu = 9, one slot: updated again
], claims={1: [f"ns above {2 * SC_}: two carries", f"update_front_lds just inside {K['UPD_LDS'] // 1024} KiB"],
           2: [f"update_front_lds just outside {K['UPD_LDS'] // 1024} KiB: the front re-assembled above an updated child"]}, small_threads=256,
    why="the only single-workgroup front of 129 columns the batch plans of clique_trees.py have")
# a third pass over the update block: leaves of 22 poses under 42 ancestor poses, nu = 126 -> 129
_scenario("22,21,21 x2: nu + 1 = 130", (22, 21, 21), 2, [
    dict(new=1, fac=[(_c(0), _n(1), "")]),
    dict(new=0, fac=[(_c(0, 1), _n(1), "")]),
    dict(new=1, fac=[(_c(0, 2), _n(2), ""), (_c(4), _n(2), "semi")]),         # the leaf's parent re-assembled: it reads the update block the leaf's update wrote
], claims={1: [f"nu + 1 above {2 * PS}: a third pass"],
           3: [f"a front re-assembled above an updated child whose update block took a third pass (nu + 1 above {2 * PS})"]}, why="the smallest three-level tree whose leaves have more than 127 update rows after one closure")
# mid: a middle front that already holds the newer pose receives the older one below it
_scenario("6,5,5 x2: a mid front", (6, 5, 5), 2, [
    dict(new=1, fac=[]),
    dict(new=1, fac=[(_c(4), _n(2), "")]),                                   # middle front 4 and the root take pose 2
    dict(new=0, fac=[(_c(0), _n(1), "")]),                                   # leaf 0 under front 4 takes pose 1: in front 4 it goes BEFORE pose 2
    dict(new=1, fac=[(_c(0, 1), _n(3), "")]),                                # (the re-assembled fronts are updated again afterwards)
], claims={1: ["a general step as one k_inc_one"], 3: ["a mid front: re-assembled, its children updated"]}, why="the smallest tree with a front between a leaf and the root")
# the tail: steps among the newest poses
_TAIL = [
    dict(new=1, fac=[]),
    dict(new=1, fac=[]),                                                    # tail_refactor from here on (the tail front was generated by the step before)
    dict(new=1, fac=[(_n(1), _n(3), "")]),
    dict(new=1, fac=[(_n(4), None, ""), (_n(3), _n(4), "")]),                # a prior on the new pose, a second factor on the odometry's pair
    dict(new=2, fac=[(_n(5), _n(2), "")]),
]
_scenario("tail steps, tail_poses = 8", (6, 5), 2, _TAIL + [
    dict(new=2, fac=[]),                                                    # 8 own poses: the front is full
    dict(new=1, fac=[]),                                                    # the next tail front opens
    dict(new=1, fac=[]),
], claims={4: ["tail_refactor with a prior on a recent pose", "tail_refactor with two factors on one pair", "tail_poses = 8"],
           6: ["a tail front brought to exactly TAIL_POSES own poses"], 7: ["the step that opens the next tail front"]}, tail_poses=8, why="a tail front of 8 poses fills up and the next opens")
_scenario("tail steps, the limits of tail_refactor", (6, 5), 2, [
    dict(new=1, fac=[]), dict(new=1, fac=[]), dict(new=1, fac=[]), dict(new=2, fac=[]), dict(new=2, fac=[]),      # poses 1 .. 7
    dict(new=1, fac=[(_n(1), _n(8), "")]),                                   # window: poses 1 .. 8 = TAILK
    dict(new=1, fac=[(_n(1), _n(9), "")]),                                   # window: poses 1 .. 9 = TAILK + 1
    dict(new=1, fac=[(_n(10 - k), _n(10), "") for k in range(2, K["TAILK"])] + [(_n(10), _n(9), "")] * (K["TAIL_MAXF"] - K["TAILK"] + 1)),      # odometry + 7 = TAIL_MAXF, window TAILK
    dict(new=1, fac=[(_n(11 - k), _n(11), "") for k in range(2, K["TAILK"])] + [(_n(11), _n(10), "")] * (K["TAIL_MAXF"] - K["TAILK"] + 1) + [(_n(11), None, "")]),      # TAIL_MAXF + 1
], claims={2: ["solve_here refused: a visited pose outside the window"], 3: ["solve_here taken"],
           6: [f"tail_refactor over a window of exactly {K['TAILK']} poses (TAILK)", "tail_poses at its default", "tail_refactor on the general path"],
           7: [f"a window of {K['TAILK'] + 1} poses: no tail_refactor", "a general step in per-level launches"],
           8: [f"tail_refactor with {K['TAIL_MAXF']} new factors (TAIL_MAXF)"], 9: [f"{K['TAIL_MAXF'] + 1} new factors among the recent poses: no tail_refactor"]},
    why="TAILK and TAIL_MAXF from either side")
# Two components: the second tree's root hangs below the tail front that owns the first tail pose of its structure, and slots are handed out in
# plain id order across the forest -- first tree, second tree, tail fronts.  Tail front 0 (poses 1 .. 8, full) sees the first tree's slot through
# its child and owns the factor between two tail poses; the second tree's slot lies between the two and passes it by: mask {0, 2}
_scenario("two trees 6,5 x2: slots {0, 2} in an updated tail front", (6, 5), 2, [
    dict(new=1, fac=[]),
    dict(new=4, fac=[]),
    dict(new=4, fac=[]),                                                     # pose 8 fills tail front 0, pose 9 opens tail front 1
    dict(new=1, fac=[(_c(0), _n(5), ""), (_d(0), _n(10), ""), (_n(5), _n(10), "")]),
], claims={4: ["a mask that is a strict, NON-CONTIGUOUS subset of the step's slots (slots {0, 2}): an updated tail front above a second component", "an updated tail front"]},
    tail_poses=8, second=((6, 5), 2), why="two trees of 17 poses: the smallest forest")


def build(name):
    """-> dict(base = arrays of the clique tree, calls = [(states of the new poses [n, 3], fa, fb, z, W, ok)] -- call 0 is the primer --, clusters)"""
    sc = SCENARIOS[name]
    rng = np.random.default_rng(SEED)
    base = CT.clique_tree(sc["levels"], sc["fan"], CT.SEED)
    cl = CT.layout(sc["levels"], sc["fan"])
    NA = len(base[0])
    cl2 = []
    if sc["second"]:                    # a second tree 30 units to the right: no factor joins the two
        b2 = CT.clique_tree(*sc["second"], CT.SEED + 1)
        cl2 = CT.layout(*sc["second"])
        st2, z2 = b2[0] + [30.0, 0, 0], b2[3].copy()
        z2[b2[2] < 0, 0] += 30.0
        base = (np.vstack([base[0], st2]), np.concatenate([base[1], b2[1] + NA]).astype(np.int32), np.concatenate([base[2], np.where(b2[2] < 0, -1, b2[2] + NA)]).astype(np.int32),
                np.vstack([base[3], z2]), np.vstack([base[4], b2[4]]))
    N0 = len(base[0])
    poses = [p for p in base[0]]
    tip = NA - 1                        # the newest pose of the chain: the first tree's last pose, then the poses added

    def node(ref):
        return cl[ref[1]][0] + ref[2] if ref[0] == "c" else NA + cl2[ref[1]][0] + ref[2] if ref[0] == "d" else N0 + ref[1]

    def rel(a, b):
        c, s = np.cos(a[2]), np.sin(a[2]); dx, dy = b[0] - a[0], b[1] - a[1]
        return np.array([c * dx + s * dy, -s * dx + c * dy, b[2] - a[2]])

    def info(flag):
        if flag == "semi":
            return np.diag([20.0, 20.0, 0.0])
        M = rng.normal(size=(3, 3)); W = M @ M.T + np.diag([20.0, 20.0, 50.0])
        W = (W + W.T) / 2
        if flag == "asym":
            W[0, 1] = np.nextafter(W[1, 0], np.inf)
        return W

    calls = []
    for step in [dict(new=1, fac=[])] + sc["steps"]:
        st, fa, fb, z, W, ok = [], [], [], [], [], []

        def add(a, b, flag):
            fa.append(a); fb.append(b)
            z.append((rel(poses[a], poses[b]) if b >= 0 else poses[a]) + rng.normal(size=3) * CT.NOISE * 0.1)
            W.append(info(flag).reshape(9)); ok.append(True if flag == "" else False if flag == "semi" else flag)
        for _ in range(step["new"]):
            last = poses[tip]
            new = np.array([last[0] + 0.3 * np.cos(last[2]), last[1] + 0.3 * np.sin(last[2]), last[2] + rng.uniform(-0.5, 0.5)])
            poses.append(new); st.append(new + rng.normal(size=3) * CT.NOISE * 0.1)
            add(tip, len(poses) - 1, "")
            tip = len(poses) - 1
        for a, b, flag in step["fac"]:
            add(node(a), node(b) if b is not None else -1, flag)
        calls.append((np.array(st).reshape(-1, 3), np.array(fa, np.int32), np.array(fb, np.int32), np.array(z).reshape(-1, 3), np.array(W).reshape(-1, 9), ok))
    return dict(base=base, calls=calls, clusters=cl, N0=N0)


def primed_arrays(B):
    """the graph the primer call plans: the base tree and the primer's pose"""
    st, fa, fb, z, W = B["base"]
    c0 = B["calls"][0]
    return np.vstack([st, c0[0]]), np.concatenate([fa, c0[1]]), np.concatenate([fb, c0[2]]), np.vstack([z, c0[3]]), np.vstack([W, c0[4]])


def designed_fronts(name):
    """the fronts of the primed base plan: the clique tree's, the root with one child more, and the primer's pose as a leaf (s = 3, u = 3)"""
    sc = SCENARIOS[name]
    d = CT.design(sc["levels"], sc["fan"])
    root = max(i for i, f in enumerate(d) if f[1] == 0)
    d[root] = (d[root][0], 0, d[root][2] + 1)
    return sorted(d + [(3, 3, 0)] + (CT.design(*sc["second"]) if sc["second"] else []))


def model_steps(name, P, **opts):
    """[(S, rows) or ("re-plan", exit)] for the calls after the primer"""
    B = build(name)
    M = Model(P, B["N0"] + 1, tail_poses=SCENARIOS[name]["tail_poses"], small_threads=SCENARIOS[name]["small_threads"], **opts)
    out = []
    for (st, fa, fb, z, W, ok) in B["calls"][1:]:
        out.append(M.step(len(st), list(zip(fa.tolist(), fb.tolist(), ok))))
    return out


def claimed(name, step, S, rows):
    """the scenario's claims of this step (1-based, after the primer) that the rows / summary do NOT show -- [] when all hold"""
    missing = []
    for c in SCENARIOS[name]["claims"].get(step, []):
        if c in ROW_CLASSES:
            if not any(r["mode"] == 1 and ROW_CLASSES[c](r) for r in rows):
                missing.append(c)
        elif c in STEP_CLASSES:
            if not STEP_CLASSES[c](rows, S):
                missing.append(c)
    return missing


def systems(name, oracle, model_dll, order_seed=None):
    """The exact linear system of every incremental call after the primer, the way tests/support/inc_exact.py builds it, on a run simulated on the
    CPU: x from the oracle, the poses written by the restated bookkeeping (aprilsam_amd_refmodel_*).  Yields (step, x).  order_seed: a seeded
    random elimination order per step instead of the oracle's own."""
    import ctypes as C
    from tests.support.inc_exact import _bind_model, _i, incremental_system
    _bind_model(model_dll)
    _dp = C.POINTER(C.c_double)
    B = build(name)
    st0, fa, fb, z, W = B["base"]
    lam0 = 1e-4
    # the batch step, then the primer (a re-plan: the same exact system as any incremental step)
    lp = st0.copy()
    _, dx, _ = oracle.batch_step(st0, fa, fb, z, W, lam=lam0)
    st = lp + dx
    q = np.where((fb < 0)[:, None], lp[fa], 0.0)          # a batch step evaluates every prior at the state it starts from
    n_batch = len(lp)
    M = C.c_void_p(model_dll.aprilsam_amd_refmodel_create())
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    try:
        model_dll.aprilsam_amd_refmodel_batch(M, len(lp), len(fa), _i(np.ascontiguousarray(fa, np.int32)), _i(np.ascontiguousarray(fb, np.int32)))
        for k, (nst, nfa, nfb, nz, nW, ok) in enumerate(B["calls"]):
            lp = np.vstack([lp, nst]); st = np.vstack([st, nst])
            fa = np.concatenate([fa, nfa]).astype(np.int32); fb = np.concatenate([fb, nfb]).astype(np.int32)
            z = np.vstack([z, nz]); W = np.vstack([W, nW])
            q = np.vstack([q, np.where((nfb < 0)[:, None], st[nfa], 0.0)])
            N = len(lp)
            model_dll.aprilsam_amd_refmodel_inc_begin(M, N, len(fa), _i(fa), _i(fb))
            zz, lam = incremental_system(lp, fa, fb, z, W, q, n_batch, lam0)
            x0 = np.ascontiguousarray(oracle.solve_system(lp, lp, fa, fb, zz, W, lam))
            x = x0 if rng is None else np.ascontiguousarray(oracle.solve_system(lp, lp, fa, fb, zz, W, lam, order=rng.permutation(N).astype(np.int32)))
            vis = np.zeros(N, np.int32)
            model_dll.aprilsam_amd_refmodel_solve_visit(M, x0.ctypes.data_as(_dp), DELTA_XY, DELTA_THETA, _i(vis))
            upd = vis == 2
            st[upd] = lp[upd] + x0[upd]                   # (the run itself follows the oracle's own order: the same systems under every order)
            yield k, x
    finally:
        model_dll.aprilsam_amd_refmodel_destroy(M)


# Largest deviation of the oracle's x from itself over three seeded random elimination orders, over every call of every scenario above, at
# max |x| of 0.11 .. 0.29: measured by tests/test_inc_designs.py (which prints the figure per scenario and holds every scenario to this bound)
# -- 2.30e-15, on "44,43 x4: ns = 129 at the LDS limit"; 1.80e-15 on "22,21,21 x2: nu + 1 = 130", below 1.5e-15 elsewhere -- rounded up to
# one digit.
INC_ORDER_DEV = 3e-15
