"""Sharded solves whose ownership map is DESIGNED: which (graph, world) pairs put the multi-rank path of csrc/solver_shard.inc.h into
the situations the lattices of tests/test_gpu_shard.py never reach.  TEST-ONLY.

CLASSES names the situations as predicates on the plan and its ownership map (owner, parent, nsb, nub, children), written from the code's
constants (CAPQ, TPB, the 64-row pass of the extend-add) and independent of the table; ENTRIES declares, per (graph, world), the classes
the entry is there for.  tests/test_shard_designs.py holds every declaration to aprilsam_amd_shard_plan on the CPU (a change of the
ordering or of shard_map cannot silently empty a class) and wants every class reached; tests/test_gpu_shard_designs.py runs every
entry through tests/support/thread_comm.py."""
import numpy as np

from aprilsam_amd import datasets
from tests.support import asym_scenarios
from tests.support import clique_trees as CT
from tests.support.consumer_graphs import lone_pose, three_components, two_components
from tests.support.mf_emulator import PlanView
from tests.support.tree_shapes import _chain, _star

K = CT.K
PASS = 64                       # rows of one pass of the extend-add (clique_trees.CLASSES)

CLIQUE_GRAPHS = ("clique 5", "6,5 x2", "22,21 x2", "23,22 x2", "43,43 x2", "44,43 x4", "86,85 x2", "6,5 x65", "5 x4 deep, fan 4",
                 "30,25,20 fan 2", "44,43,43 fan 2", "16 x6 deep", "mixed leaves 200,130,64 under 64")
OTHER_GRAPHS = {
    "star_70": lambda lib: _star(70, 2),
    "chain_300": lambda lib: _chain(300, 3),
    "random_300": lambda lib: datasets.random_pose_graph(300, 200, 3),           # (with_prior inside: the prior is part of it)
    "two_components": lambda lib: two_components()[0],
    "three_components": lambda lib: three_components()[0],
    "lone_pose": lambda lib: lone_pose(),
    "asym_batch": lambda lib: asym_scenarios.batch_graph(),
    "lattice_24": lambda lib: lib.lattice_arrays(24),
    "m3500": lambda lib: datasets.m3500_batch(),
}
GRAPHS = CLIQUE_GRAPHS + tuple(OTHER_GRAPHS)
FEW_WORLDS = ("m3500", "16 x6 deep")          # more than 500 poses: worlds 2, 3 and 8
WORLDS, WORLDS_FEW = (2, 3, 4, 5, 8), (2, 3, 8)
MAX_POSES = 3500

_ARR, _PLAN = {}, {}


def arrays(lib, name):
    if name not in _ARR:
        if name in CLIQUE_GRAPHS:
            levels, fan, _, _ = CT.CASES[name]
            arr = CT.clique_tree(levels, fan, CT.SEED)
        else:
            arr = OTHER_GRAPHS[name](lib)
        arr = tuple(np.ascontiguousarray(a) for a in arr)
        for a in arr:
            a.setflags(write=False)
        assert len(arr[0]) <= MAX_POSES
        _ARR[name] = arr
    return _ARR[name]


def worlds_of(name):
    return WORLDS_FEW if name in FEW_WORLDS else WORLDS


def plan(lib, name):
    """the library's plan of the graph with the ownership maps of every world the graph runs at (and world 1)"""
    if name not in _PLAN:
        arr = arrays(lib, name)
        _PLAN[name] = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2], shard_worlds=(1,) + tuple(worlds_of(name)))
    return _PLAN[name]


class Map:
    """what the predicates see: the plan's tree and one world's ownership"""

    def __init__(self, P, world, W=None):
        self.world = int(world)
        self.xfer, self.bcast, self.owner = P.shard[world]
        self.parent, self.nsb, self.nub = P.front_parent, P.front_nsb, P.front_nub
        self.children = [P.ch_idx[int(P.ch_ptr[t]):int(P.ch_ptr[t + 1])] for t in range(P.nF)]
        self.W = W
        par = np.where(self.parent >= 0, self.parent, 0)
        self.ghost = (self.parent >= 0) & (self.owner[par] != self.owner)          # per front: its parent lives on another rank
        self.ghost_u1 = 3 * self.nub[self.ghost] + 1                               # rows of the ghosts' update blocks with the right-hand side
        self.remote_children = np.array([int(np.sum(self.ghost[c])) for c in self.children])

    def primary(self, t):
        """the children of front t that upload_plan makes prim1 / prim2: the largest update block, then the largest of the rest (the first of
        equals, in the plan's child order)"""
        ch = [int(c) for c in self.children[t] if self.nub[c] > 0]
        if not ch:
            return []
        best = max(ch, key=lambda c: (self.nub[c], -ch.index(c)))
        rest = [c for c in ch if c != best]
        return [best] + ([max(rest, key=lambda c: (self.nub[c], -rest.index(c)))] if rest else [])

    def primary_ghosts(self):
        return [c for t in range(len(self.parent)) for c in self.primary(t) if self.ghost[c]]

    def pool_doubles(self, rank):
        """doubles of a rank's front pool (shard_begin_impl): the owned fronts' arrays, then the ghosts' update blocks, each on a 32-double boundary"""
        run = 0
        for t in np.flatnonzero(self.owner == rank):
            m = 3 * int(self.nsb[t] + self.nub[t])
            run = ((run + 31) & ~31) + (m + 3) * m
        for t in np.flatnonzero(self.ghost):
            if self.owner[self.parent[t]] == rank:
                u = 3 * int(self.nub[t])
                run = ((run + 31) & ~31) + (u + 3) * u
        return run


def _u1(pred):
    return lambda M: bool(np.any(pred(M.ghost_u1)))


# id -> (what, predicate on a Map)
CLASSES = {
    "idle": ("a rank that owns nothing", lambda M: len(set(M.owner.tolist())) < M.world),
    "prim": ("a ghost that is its parent's primary child", lambda M: len(M.primary_ghosts()) > 0),
    "u<64": ("ghost u + 1 < 64: less than one pass", _u1(lambda v: v < PASS)),
    "u=64": ("ghost u + 1 = 64: exactly one pass", _u1(lambda v: v == PASS)),
    "u67": ("ghost 64 < u + 1 <= 67: a second pass, nearly empty", _u1(lambda v: (v > PASS) & (v <= PASS + 3))),
    "u130": ("ghost 128 < u + 1 <= 131: rest()", _u1(lambda v: (v > 2 * PASS) & (v <= 2 * PASS + 3))),
    "u3-4": ("ghost 131 < u + 1 < TPB: three and four passes", _u1(lambda v: (v > 2 * PASS + 3) & (v < K["TPB"]))),
    "u=TPB": ("ghost u + 1 = TPB: exactly one trip of k_pack_update's column loop", _u1(lambda v: v == K["TPB"])),
    "u>TPB": ("ghost TPB < u + 1 <= TPB + 3: a second trip, nearly empty", _u1(lambda v: (v > K["TPB"]) & (v <= K["TPB"] + 3))),
    "half": ("CAPQ / 2 or more remote children of one front", lambda M: bool(np.any(M.remote_children >= K["CAPQ"] // 2))),
    "refill": ("remote children of a front with more than CAPQ children (staged child records refilled)",
               lambda M: any(len(c) > K["CAPQ"] and M.remote_children[t] > 0 for t, c in enumerate(M.children))),
    "roots": ("several roots", lambda M: int(np.sum(M.parent < 0)) > 1),
    "odd": ("a world that is no power of two", lambda M: M.world & (M.world - 1) != 0),
    "asym": ("asymmetric W", lambda M: M.W is not None and not np.array_equal(M.W.reshape(-1, 3, 3), M.W.reshape(-1, 3, 3).transpose(0, 2, 1))),
}


def classes_of(lib, name, world):
    W = arrays(lib, name)[4]
    M = Map(plan(lib, name), world, W)
    return [c for c, (_, pred) in CLASSES.items() if pred(M)]


# ------------------------------------------------------------------------------------------------------
# the entries: graph -> world -> the classes the entry reaches, ALL of them (tests/test_shard_designs.py wants the library's plan to give
# exactly these: an entry can neither lose a class nor gain one unnoticed)
# ------------------------------------------------------------------------------------------------------
ENTRIES = {
    'clique 5': {2: 'idle', 3: 'idle odd', 4: 'idle', 5: 'idle odd', 8: 'idle'},
    '6,5 x2': {2: 'prim u<64', 3: 'idle prim u<64 odd', 4: 'idle prim u<64', 5: 'idle prim u<64 odd', 8: 'idle prim u<64'},
    '22,21 x2': {2: 'prim u=64', 3: 'idle prim u=64 odd', 4: 'idle prim u=64', 5: 'idle prim u=64 odd', 8: 'idle prim u=64'},
    '23,22 x2': {2: 'prim u67', 3: 'idle prim u67 odd', 4: 'idle prim u67', 5: 'idle prim u67 odd', 8: 'idle prim u67'},
    '43,43 x2': {2: 'prim u130', 3: 'idle prim u130 odd', 4: 'idle prim u130', 5: 'idle prim u130 odd', 8: 'idle prim u130'},
    '44,43 x4': {2: 'prim u130', 3: 'idle prim u130 odd', 4: 'idle prim u130', 5: 'idle prim u130 odd', 8: 'idle prim u130'},
    '86,85 x2': {2: 'prim u=TPB', 3: 'idle prim u=TPB odd', 4: 'idle prim u=TPB', 5: 'idle prim u=TPB odd', 8: 'idle prim u=TPB'},
    '6,5 x65': {2: 'prim u<64 half refill', 3: 'idle prim u<64 half refill odd', 4: 'idle prim u<64 half refill', 5: 'idle prim u<64 half refill odd',
                8: 'idle prim u<64 half refill'},
    '5 x4 deep, fan 4': {2: 'prim u<64', 3: 'prim u<64 odd', 4: 'prim u<64', 5: 'prim u<64 odd', 8: 'prim u<64'},
    '30,25,20 fan 2': {2: 'prim u<64', 3: 'prim u<64 u3-4 odd', 4: 'prim u<64 u3-4', 5: 'idle prim u<64 u3-4 odd', 8: 'idle prim u<64 u3-4'},
    '44,43,43 fan 2': {2: 'prim u130', 3: 'prim u130 u>TPB odd', 4: 'prim u130 u>TPB', 5: 'idle prim u130 u>TPB odd', 8: 'idle prim u130 u>TPB'},
    '16 x6 deep': {2: 'prim u<64', 3: 'prim u<64 odd', 8: 'prim u<64 u3-4'},
    'mixed leaves 200,130,64 under 64': {2: 'prim u3-4', 3: 'idle prim u3-4 odd', 4: 'idle prim u3-4', 5: 'idle prim u3-4 odd', 8: 'idle prim u3-4'},
    'star_70': {2: 'prim u<64 half refill', 3: 'idle prim u<64 half refill odd', 4: 'idle prim u<64 half refill', 5: 'idle prim u<64 half refill odd',
                8: 'idle prim u<64 half refill'},
    'chain_300': {2: 'prim u<64', 3: 'prim u<64 odd', 4: 'prim u<64', 5: 'prim u<64 odd', 8: 'prim u<64'},
    'random_300': {2: 'prim u<64 u3-4', 3: 'prim u<64 u3-4 odd', 4: 'prim u<64 u3-4', 5: 'idle prim u<64 u3-4 odd', 8: 'idle prim u<64 u3-4'},
    'two_components': {2: 'prim u<64 u3-4 roots', 3: 'prim u<64 u3-4 roots odd', 4: 'prim u<64 u3-4 roots', 5: 'prim u<64 u3-4 roots odd', 8: 'prim u<64 u3-4 roots'},
    'three_components': {2: 'prim u<64 u3-4 roots', 3: 'prim u<64 u3-4 roots odd', 4: 'prim u<64 u3-4 roots', 5: 'prim u<64 u3-4 roots odd', 8: 'prim u<64 u3-4 roots'},
    'lone_pose': {2: 'idle', 3: 'idle odd', 4: 'idle', 5: 'idle odd', 8: 'idle'},
    'asym_batch': {2: 'prim u<64 u3-4 asym', 3: 'prim u<64 u3-4 odd asym', 4: 'prim u<64 u3-4 asym', 5: 'prim u<64 u3-4 odd asym', 8: 'prim u<64 u3-4 asym'},
    'lattice_24': {2: 'prim', 3: 'prim u=64 odd', 4: 'prim u=64', 5: 'prim u<64 u=64 odd', 8: 'prim u<64 u=64'},
    'm3500': {2: 'prim u<64', 3: 'prim u<64 odd', 8: 'prim u<64 u67'},
}
ALL = [(name, w) for name in GRAPHS for w in worlds_of(name)]


def declared(name, world):
    return ENTRIES[name][world].split()


def ident(entry):
    return f"{entry[0]} @{entry[1]}"


# the entries that also run under the option sets that change the form of the kernels which read ghosts and back-substitute top fronts:
# every entry with a primary ghost -- among them the 259-row ghost ('44,43,43 fan 2' from 3 ranks on) and the fronts of 32 and 35 remote
# children ('6,5 x65', 'star_70')
OPTION_ENTRIES = [e for e in ALL if "prim" in declared(*e)]
THREE_ITERATIONS = [("random_300", 3), ("two_components", 3), ("m3500", 3)]


def describe(lib):
    """prints the table below as the library's plans give it (for whoever has to re-declare it after a deliberate change of the ordering)"""
    for name in GRAPHS:
        print(f"    {name!r}: {{" + ", ".join(f"{w}: {' '.join(classes_of(lib, name, w))!r}" for w in worlds_of(name)) + "},")
