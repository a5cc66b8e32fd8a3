"""Every consumer of the retained factor after every event that touches the graph, the param or the graph's device copy (DESIGN.md section
25; tests/support/retained_contract.py holds the scene, the Systems, the consumers, the events and the table EXPECTED).

Per event: two successful april_graph_cholesky calls (they leave S0 and a captured graph), the event, then every consumer.  A cell that
names a System must succeed, pass that consumer's existing checker against the dense reference of THAT system -- built from the test's own
arrays and the l_points the factorising call left -- and must not pass it against the system it replaced.  A cell that names a code must
return exactly that code, record it in aprilsam_amd_last_error, leave every sentinel in its outputs, and leave the plan fields of stats, the
count of selected inversions and the graph's states, l_points and delta_X bit for bit.  Every event ends with one more april_graph_cholesky,
which must succeed with a normal-equation residual below 1e-10: a refusal never costs the next call anything.

A consumer that answers from a stale factor returns the previous system's correct numbers: finite, plausible, reproducible.  The margins by
which each checker tells the systems apart are asserted on the CPU (tests/test_retained_contract_model.py)."""
import pytest

from tests.support import retained_contract as rc
from tests.support.kernel_paths import KERNEL_PATHS

pytestmark = pytest.mark.gpu


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _run(lib, oracle, event, **opts):
    try:
        bad, record = rc.run_event(lib, event, oracle, print, **opts)
    except rc.DeviceTrouble as e:
        pytest.exit(f"a HIP call failed, nothing more runs on this device: {e}", returncode=3)
    assert not bad, "\n".join([f"{event} {_ids(opts)}:"] + bad)
    return record


@pytest.mark.parametrize("event", list(rc.EVENTS))
def test_every_consumer_after_the_event(lib, oracle, event):
    _run(lib, oracle, event)


@pytest.mark.parametrize("event", list(rc.FAM_EVENTS))
def test_every_consumer_after_the_family_event(lib, oracle, event):
    """the families scene: a Cauchy closure, a max-mixture closure, a range-bearing landmark seen from two poses and a dense Gaussian factor;
    the thirteen consumers and gate_polar, associate_polar, robust_weights, max_selected"""
    _run(lib, oracle, event)


@pytest.mark.parametrize("event", list(rc.EVENTS) + list(rc.FAM_EVENTS))
def test_replay_changes_no_bit_and_no_code(lib, oracle, event):
    """the same case without captured graphs: every return code and every output of every consumer, and the closing call's states and
    delta_X, are bitwise those of the run with them"""
    first = _run(lib, oracle, event)
    second = _run(lib, oracle, event, use_graph=0)
    assert [(n, r) for n, r, _ in first] == [(n, r) for n, r, _ in second]
    for (name, _, a), (_, _, b) in zip(first, second):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], (event, name, k)


@pytest.mark.parametrize("opts", [KERNEL_PATHS[0], KERNEL_PATHS[-1], dict(pool_poison=1), dict(pool_guard=64)], ids=_ids)
@pytest.mark.parametrize("event", ["03_third_call", "10_other_param_steps", "18_resident_ended", "24_inc_fast", "28b_reduced_solved"] + rc.FAM_NEW_SYSTEM_EVENTS)
def test_events_that_rewrite_fronts_on_other_kernel_paths(lib, oracle, event, opts):
    """poison fills what a later step hands over: a consumer that reads a front the event's step rewrote shows NaN instead of the last
    step's numbers; guard bands move every front's offset; the first and the last option set of the kernel-path matrix"""
    _run(lib, oracle, event, **opts)
