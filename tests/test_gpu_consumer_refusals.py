"""What "one admission sequence" means from outside: every consumer of the retained factor, asked in each state in
which the sequence refuses, gives the same answer in the same words.

The sequence is: a sharded param (-12) -> a node fixed or freed since the factorisation (drops the factor) -> no retained factor (-1) ->
a factor made from an asymmetric information matrix (-12).  Scene: the 40-pose loop of tests/support/retained_contract.scene().  States:

    fresh            a param no solver call has used
    resident_open    a resident loop that is open
    own_call_failed  the param's last call failed not-positive-definite (retained_contract.ev_own_call_fails)
    asymmetric       the graph holds one factor with an asymmetric W (the text loader's form, tests/test_gpu_asymmetric_w.py)
    sharded          aprilsam_amd_shard_begin has succeeded on the param (one rank of one: tests/test_gpu_shard.py,
                     test_rccl_transport_on_one_rank, shows that this needs one device only)

Each state is crossed with every entry of retained_contract.CONSUMERS and gate_polar, associate_polar, marginal_prior and
factorised_nodes.  Per cell: the return code, aprilsam_amd_last_error's code, the message -- exactly "<who>: <reason>", <reason> from the
five-entry table REASON, <who> from the table WHO -- and every output still at its sentinel.  The cells that are no refusals are written
down as what they are: aprilsam_amd_factorised_nodes takes no graph, records no error and asks only whether a factor is retained (the node
count on the asymmetric graph; -1 on a sharded param, which has factorised nothing before its first iteration); april_graph_cholesky_inc
and _inc_solver are void and return silently -- but for the asymmetric graph, where they hold a healthy factor and the header defines
no refusal (retained_contract.EXPECTED: "step" / "undefined"): not run there.  The precedence case pins the order: an open resident loop
on the asymmetric graph reports the missing factor, not the asymmetry.

Both tables were filled from the library as it was before the consumers shared one admission point, and this file passed against that
library unchanged."""
import ctypes as C

import numpy as np
import pytest

from tests.support import polar_gate_model as pgm
from tests.support import retained_contract as rc

pytestmark = pytest.mark.gpu

NO_FACTOR = (-1, "no retained factor (no successful solver call since the param was created or last failed)")
REASON = {"fresh": NO_FACTOR,
          "resident_open": NO_FACTOR,
          "own_call_failed": NO_FACTOR,
          "asymmetric": (-12, "the factorised graph holds factors with an asymmetric information matrix"),
          "sharded": (-12, "sharded params are not supported")}
# the name each consumer answers under.  marginals_joint: aprilsam_amd_marginals_joint reports under aprilsam_amd_marginals' name (only its
# "null node list" message carries its own)
WHO = {"marginals_all": "aprilsam_amd_marginals", "marginals_list": "aprilsam_amd_marginals", "marginals_joint": "aprilsam_amd_marginals",
       "joint_any": "aprilsam_amd_marginals_joint_any", "gate_xyt": "aprilsam_amd_gate_xyt", "solve": "aprilsam_amd_solve",
       "marginals_cross": "aprilsam_amd_marginals_cross", "relative_covariances": "aprilsam_amd_relative_covariances",
       "factor_audit": "aprilsam_amd_factor_audit", "marginal_prior": "aprilsam_amd_marginal_prior", "gate_polar": "aprilsam_amd_gate_polar",
       "associate_polar": "aprilsam_amd_associate_polar"}
# no refusals: (return value, last error's code, message) per state, "*" for every state not named
NOT_REFUSED = {"factorised_nodes": {"asymmetric": (rc.N0, 0, ""), "*": (-1, 0, "")},
               "cholesky_inc": {"*": (0, 0, ""), "asymmetric": None}, "cholesky_inc_solver": {"*": (0, 0, ""), "asymmetric": None}}


class _Single(rc.Consumer):
    """one call of one entry point on sentinel-prefilled outputs (the contract's GateXyt and the polar consumers make a second call, whose
    message would replace the first's)"""

    def __init__(self, name, call):
        self.name, self.call = name, call


def _gate_xyt(lib, g, p, Nb):
    n = len(rc.GATE_A)
    d2, S = rc._sent(n), rc._sent(n, 3, 3)
    return lib.dll.aprilsam_amd_gate_xyt(g.ptr, p.ptr, n, rc.i_(rc.GATE_A), rc.i_(rc.GATE_B), rc.d_(rc.GATE_Z), rc.d_(rc.GATE_W), rc.d_(d2), rc.d_(S)), dict(d2=d2, S=S)


POLAR = [(rc.pm.RANGE_BEARING, 12, 30, [1.9, 0.4], [[2500.0, 30.0], [30.0, 10000.0]]), (rc.pm.RANGE, 5, 20, [6.0], [[2500.0]])]
OBSERVER, LANDMARKS = 13, np.array([30, 12, 25], np.int32)


def _gate_polar(lib, g, p, Nb):
    n = len(POLAR)
    a, b = np.array([c[1] for c in POLAR], np.int32), np.array([c[2] for c in POLAR], np.int32)
    kind, z, W = rc._polar_arrays([(c[0], c[3], c[4]) for c in POLAR])
    d2, S = rc._sent(n), rc._sent(n, 2, 2)
    return lib.dll.aprilsam_amd_gate_polar(g.ptr, p.ptr, n, rc.i_(a), rc.i_(b), rc.i_(kind), rc.d_(z), rc.d_(W), rc.d_(d2), rc.d_(S)), dict(d2=d2, S=S)


def _associate_polar(lib, g, p, Nb):
    m, L = len(POLAR), len(LANDMARKS)
    kind, z, W = rc._polar_arrays([(c[0], c[3], c[4]) for c in POLAR])
    d2, best, b1, b2 = rc._sent(m, L), np.full(m, -7, np.int32), rc._sent(m), rc._sent(m)
    r = lib.dll.aprilsam_amd_associate_polar(g.ptr, p.ptr, OBSERVER, m, rc.i_(kind), rc.d_(z), rc.d_(W), L, rc.i_(LANDMARKS), pgm.CHI2_1_999, pgm.CHI2_2_999,
                                             rc.d_(d2), rc.i_(best), rc.d_(b1), rc.d_(b2))
    return r, dict(d2=d2, best=np.where(best == -7, rc.SENT, best.astype(float)), d2_best=b1, d2_second=b2)


OWN = {"gate_xyt": _Single("gate_xyt", _gate_xyt), "gate_polar": _Single("gate_polar", _gate_polar),
       "associate_polar": _Single("associate_polar", _associate_polar)}
CONSUMERS = [OWN.get(c.name, c) for c in rc.CONSUMERS] + [OWN["gate_polar"], OWN["associate_polar"]]
assert {"marginal_prior", "factorised_nodes"} <= {c.name for c in CONSUMERS} and {c.name for c in CONSUMERS} == set(WHO) | set(NOT_REFUSED)


def _asymmetric_scene():
    """the scene with the last closure's W as the reference's text loader leaves a correlated one: upper triangle filled, lower zero"""
    sc = rc.scene()
    sc["W"][-1, [3, 6, 7]] = 0.0
    return sc


def _shard(ctx):
    d = ctx.lib.dll
    d.aprilsam_amd_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    d.aprilsam_amd_shard_end.argtypes = [C.c_void_p]
    g, p = C.cast(ctx.g.ptr, C.c_void_p), C.cast(ctx.p.ptr, C.c_void_p)
    assert d.aprilsam_amd_shard_begin(g, p, 0, 1) == 0, ctx.lib.last_error()
    ctx.cleanup.append(lambda: d.aprilsam_amd_shard_end(p))


# state -> (the scene, whether two successful calls come first, what then brings the state about)
STATES = {"fresh": (rc.scene, False, lambda ctx: None),
          "resident_open": (rc.scene, True, rc.ev_resident_open),
          "own_call_failed": (rc.scene, True, rc.ev_own_call_fails),
          "asymmetric": (_asymmetric_scene, True, lambda ctx: None),
          "sharded": (rc.scene, False, _shard)}


def _cells(lib, state, scene, warm, enter):
    """every consumer in one state -> the complaints"""
    bad = []
    code, reason = REASON[state]
    ctx = rc.Ctx(lib, sc=scene())
    try:
        if warm:
            ctx.start()
        enter(ctx)
        for cons in CONSUMERS:
            if cons.name in NOT_REFUSED and NOT_REFUSED[cons.name].get(state, True) is None:
                continue
            lib.clear_error()
            got_rc, out = cons.call(lib, ctx.g, ctx.p, ctx.g.n_nodes)
            err, msg = lib.last_error()
            if err in (-9, -10):
                pytest.exit(f"a HIP call failed, nothing more runs on this device: {state}, {cons.name}: {msg}", returncode=3)
            if cons.name in NOT_REFUSED:
                row = NOT_REFUSED[cons.name]
                want = row.get(state, row["*"])
                got = (int(out["n"][0]) if cons.name == "factorised_nodes" else got_rc, err, msg)
                if cons.name != "factorised_nodes" and not cons.untouched(out):
                    bad.append(f"{state}, {cons.name}: wrote into the graph")
            else:
                want, got = (code, code, f"{WHO[cons.name]}: {reason}"), (got_rc, err, msg)
                if not cons.untouched(out):
                    bad.append(f"{state}, {cons.name}: a refusal wrote into its outputs")
            print(f"{state:16s} {cons.name:22s} {got}")
            if got != want:
                bad.append(f"{state}, {cons.name}: {got} where the tables say {want}")
        for undo in reversed(ctx.cleanup):
            undo()
    finally:
        ctx.destroy()
    return bad


@pytest.mark.parametrize("state", list(STATES))
def test_every_consumer_refuses_in_the_same_words(lib, state):
    bad = _cells(lib, state, *STATES[state])
    assert not bad, "\n".join(bad)


def test_a_missing_factor_is_reported_before_an_asymmetric_one(lib):
    """an open resident loop on the asymmetric graph: both refusals apply, the sequence asks for the factor first"""
    bad = _cells(lib, "resident_open", _asymmetric_scene, True, rc.ev_resident_open)
    assert not bad, "\n".join(bad)
