"""The designed incremental scenarios of tests/support/inc_designs.py on the CPU: every scenario's frozen base plans as designed (the library's
own plan of the primed graph, PlanView), every class of the table is claimed by a scenario whose declared rows show it, and the reference the GPU
test compares with (the oracle, on the exact incremental system of every call) deviates from itself over elimination orders by no more than
INC_ORDER_DEV -- the figure the GPU test's rounding-size bar is made of."""
import numpy as np
import pytest

from tests.support import inc_designs as ID
from tests.support.mf_emulator import PlanView

_PLANS = {}


def plan_of(lib, name):
    if name not in _PLANS:
        arr = ID.primed_arrays(ID.build(name))
        _PLANS[name] = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2])
    return _PLANS[name]


@pytest.mark.parametrize("name", list(ID.SCENARIOS))
def test_the_base_plan_is_the_designed_one(lib, name):
    P = plan_of(lib, name)
    fronts = sorted(zip((3 * P.front_nsb).tolist(), (3 * P.front_nub).tolist(), np.diff(P.ch_ptr).tolist()))
    assert fronts == ID.designed_fronts(name)
    B = ID.build(name)
    assert int(P.front_nsb[int(np.searchsorted(P.front_first, P.pos[B["N0"]], side="right")) - 1]) == 1          # the primer's pose: a front of its own
    assert len(B["base"][0]) <= 400 and len(B["calls"]) <= 10           # (nine calls and the primer: "tail steps, the limits of tail_refactor", four limits behind five calls that bring the front to seven poses)


def _describe(step):
    if step[0] == "re-plan":
        return f"re-plan (exit {step[1]})"
    S, rows = step
    what = "tail_refactor" if S["tail_fast"] else "general"
    return what + " " + " ".join(f"[{r['front']}{'U' if r['mode'] else 'A'} ns {r['ns']} nu {r['nu_o']}->{r['nu']} mask {r['mask']:b} ch {r['n_ch']}"
                                 f"{' in place' if r['inplace'] else ''}{' mid' if r['mid'] else ''}]" for r in rows)


@pytest.mark.parametrize("name", list(ID.SCENARIOS))
def test_every_scenario_shows_what_it_claims(lib, name):
    steps = ID.model_steps(name, plan_of(lib, name))
    print()
    for k, step in enumerate(steps, 1):
        print(f"{name} | call {k}: {_describe(step)}")
    sc = ID.SCENARIOS[name]
    assert all(1 <= k <= len(steps) for k in sc["claims"])
    for k, step in enumerate(steps, 1):
        assert step[0] != "re-plan", (name, k, step)
        assert ID.claimed(name, k, *step) == [], (name, k)
        assert all(c in ID.CLASSES for c in sc["claims"].get(k, [])), (name, k)


def test_every_class_is_claimed():
    where = {c: [] for c in ID.CLASSES}
    for name, sc in ID.SCENARIOS.items():
        for k, cs in sc["claims"].items():
            for c in cs:
                where[c].append(f"{name} (call {k})")
    print()
    for c, w in where.items():
        print(f"{c}: {', '.join(w) if w else 'NOTHING'}")
    for c, why in ID.NOT_REACHED.items():
        print(f"NOT REACHED | {c}: {why}")
    for c, w in where.items():
        assert w, c


def test_the_constants_are_the_headers():
    """every constant the classes are made of was found in the headers (the regexes of inc_designs._constants matched), and the classes use them"""
    K = ID.K
    for name in ("UPD_MAXF", "UPD_MAXC", "TAIL_MAXF", "TAILQ", "TAILK", "INL_PATCHES", "FS_BLOCK", "SCAN", "PASS", "UPD_LDS"):
        assert isinstance(K[name], int) and K[name] > 0, name
    assert any(str(K["FS_BLOCK"] + 1) in c for c in ID.ROW_CLASSES) and any(str(K["TAILK"]) in c for c in ID.STEP_CLASSES)


@pytest.mark.parametrize("name", list(ID.SCENARIOS))
def test_the_oracle_deviates_from_itself_by_rounding_only(lib, oracle, name):
    own = [x for _, x in ID.systems(name, oracle, lib.dll)]
    dev, top = 0.0, 0.0
    for seed in (ID.SEED + 1, ID.SEED + 2, ID.SEED + 3):
        for (k, x), x0 in zip(ID.systems(name, oracle, lib.dll, order_seed=seed), own):
            dev = max(dev, float(np.max(np.abs(x - x0))))
            top = max(top, float(np.max(np.abs(x0))))
    print(f"\nINC_ORDER_DEV | {name}: deviation over three random orders {dev:.2e}, max |x| {top:.3f}, {len(own)} calls")
    assert dev <= ID.INC_ORDER_DEV, (name, dev)
