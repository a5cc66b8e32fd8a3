"""The clique trees of tests/support/clique_trees.py on the CPU: every case plans as designed (the library's own plan, PlanView, as
tests/test_front_census.py reads it -- with the pose positions as the hint the solver gives the dissection), the union of the cases fills
every shape class the kernels treat differently, and the reference the GPU tests compare with (the oracle) stays far inside their
tolerances on its own: its normal-equation residual, and its deviation from itself over random elimination orders (ORDER_DEV)."""
import numpy as np
import pytest

from tests.support import clique_trees as CT
from tests.support.mf_emulator import PlanView
from tests.support.normal_eq import normal_equation_residual

LAM = 1e-4
RES_RTOL = 1e-10          # tests/test_gpu_normal_eq.py


@pytest.fixture(scope="module")
def plans(lib):
    out = {}
    for name, (levels, fan, _, _) in CT.CASES.items():
        arr = CT.clique_tree(levels, fan, CT.SEED)
        out[name] = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2])
    return out


def _fronts(P):
    return 3 * P.front_nsb, 3 * P.front_nub, np.diff(P.ch_ptr)


@pytest.mark.parametrize("name", list(CT.CASES))
def test_the_plan_is_the_designed_one(plans, name):
    s, u, ch = _fronts(plans[name])
    assert sorted(zip(s.tolist(), u.tolist(), ch.tolist())) == CT.CASES[name][2]


def test_the_design_rule_itself():
    """a cluster of a poses under ancestors of b poses in all: (3a, 3b, children)"""
    assert CT.design((44, 43, 43), 2) == sorted([(132, 258, 0)] * 4 + [(129, 129, 2)] * 2 + [(129, 0, 2)])
    assert CT.design(((200, 130, 64), 64), 3) == sorted([(600, 192, 0), (390, 192, 0), (192, 192, 0), (192, 0, 3)])
    assert CT.design((5,), 1) == [(15, 0, 0)]


def test_the_cases_fill_every_shape_class(plans):
    counts = {c: {} for c in CT.CLASSES}
    levelled = []
    for name, P in plans.items():
        s, u, ch = _fronts(P)
        for c, f in CT.CLASSES.items():
            n = int(np.sum(f(s, u, ch)))
            if n:
                counts[c][name] = n
        for l in range(P.nLevels):
            if CT.level_has_unequal_big(s[P.lev_fronts[int(P.lev_ptr[l]):int(P.lev_ptr[l + 1])]]):
                levelled.append(name)
    print()
    for c, where in counts.items():
        print(f"{c}: {', '.join(where) if where else 'NOTHING'}")
    print(f"{CT.LEVEL_CLASS}: {', '.join(levelled) if levelled else 'NOTHING'}")
    for c, where in counts.items():
        assert where, c
    assert levelled, CT.LEVEL_CLASS


def _random_orders(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.permutation(n).astype(np.int32) for _ in range(3)]


@pytest.mark.parametrize("name", list(CT.CASES))
def test_the_oracle_stays_inside_the_tolerances_on_its_own(oracle, name):
    levels, fan, _, _ = CT.CASES[name]
    arr = CT.clique_tree(levels, fan, CT.SEED)
    _, dx, _ = oracle.batch_step(*arr, lam=LAM)
    out = normal_equation_residual(arr[0], arr[1], arr[2], arr[3], arr[4], dx, LAM)
    dev = 0.0
    for order in _random_orders(len(arr[0]), CT.SEED + 1):
        dev = max(dev, float(np.max(np.abs(oracle.batch_step(*arr, lam=LAM, order=order)[1] - dx))))
    print(f"\n{name}: oracle residual {out['rel_max']:.2e}, deviation over three random orders {dev:.2e}, max |dx| {np.max(np.abs(dx)):.2f}")
    assert out["rel_max"] < RES_RTOL / 100, out
    assert dev <= CT.ORDER_DEV, dev
