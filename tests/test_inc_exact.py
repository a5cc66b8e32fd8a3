"""The per-step exact checker of the incremental path (tests/support/inc_exact.py), pinned on the CPU against the unmodified reference
(oracle/_ref): the reference passes it on every scenario the GPU tests drive through it, and it rejects host-side offsets of returned
states far below what the chi^2-trace comparisons notice.  Skips when oracle/_ref is absent."""
import numpy as np
import pytest

from aprilsam_amd import datasets, harness
from tests.conftest import golden
from tests.support.inc_exact import IncExact
import tests.test_gpu_parity as T

# the reference's distance to the exact solve of its incremental system, measured here: 2.8e-11 on the demo's first 700 poses and at most
# 5e-13 on the growth scenarios, except 140 steps of random growth without a fall-back (seed 2), where the poses drift far from their
# l_points: 1.9e-10.  The checker's bar on the GPU is 1e-9.
REF_BOUND = 1e-10
SCENARIOS = {
    "demo700": (lambda L: harness.run_demo(L, datasets.m3500_arrays(), max_poses=700), REF_BOUND),
    "tutorial": (lambda L: harness.run_tutorial(L), REF_BOUND),
    "random_growth_1": (lambda L: T._random_growth(L, 1, 140, 25), REF_BOUND),
    "random_growth_2": (lambda L: T._random_growth(L, 2, 140, 10 ** 6), 3e-10),
    "random_growth_3": (lambda L: T._random_growth(L, 3, 140, 8), REF_BOUND),
    "recent_pose_growth": (lambda L: T._recent_pose_growth(L, 12, 120, 40, 28), REF_BOUND),
    "late_priors": (lambda L: T._growth_with_late_priors(L), REF_BOUND),
    "batch_every_37": (lambda L: harness.run_demo(L, datasets.m3500_arrays(), max_poses=300, batch_every=37), REF_BOUND),
}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_the_reference_passes_the_checker(lib, reflib, oracle, name):
    run, bound = SCENARIOS[name]
    chk = IncExact(reflib, oracle, model_lib=lib, log=print)
    run(chk)
    r = chk.report
    print(f"reference, {name}: {chk.summary()}")
    assert r["failures"] == 0 and r["checked"] == r["inc"] > 0
    assert r["inc_state"] <= bound and r["inc_delta"] <= bound and r["batch_res"] < 1e-12
    if name == "demo700":
        assert r["fallback_nodes"] == [232, 350, 508, 591]


def _offset(poses, by, from_step):
    def after_call(k, g, written):
        if written is not None and k >= from_step:
            for i in poses(written):
                s = g.states_of(i)
                g.set_state(int(i), [s[0] + by, s[1] + by, s[2] + by])
    return after_call


def test_an_offset_of_1e_8_on_one_written_pose_of_one_step_is_rejected(lib, reflib, oracle):
    """host-side arithmetic on a state the reference returned: one pose the step wrote, step 260 of the demo only"""
    hit = []

    def one(written):
        hit.append(int(np.nonzero(written)[0][0]))
        return hit[-1:]
    after = _offset(one, 1e-8, 260)
    only_260 = lambda k, g, w: after(k, g, w) if k == 260 else None     # noqa: E731
    chk = IncExact(reflib, oracle, model_lib=lib, strict=False, after_call=only_260)
    harness.run_demo(chk, datasets.m3500_arrays(), max_poses=300)
    r = chk.report
    print(f"1e-8 on pose {hit} at step 260: {r['first_failure']}")
    assert hit and r["failures"] == 1 and "step 260" in r["first_failure"]
    assert 0.9e-8 < r["inc_state"] < 1.1e-8
    with pytest.raises(AssertionError, match="step 260"):          # (strict, as the GPU tests run it)
        harness.run_demo(IncExact(reflib, oracle, model_lib=lib, after_call=only_260), datasets.m3500_arrays(), max_poses=300)


def test_a_1e_6_offset_passes_the_chi2_trace_bar_and_is_rejected(lib, reflib, oracle):
    """Why the incremental path needs this checker: every pose every step writes, moved by 1e-6 in x, y and theta from step 250 on, keeps
    the chi^2 trace of the first 420 poses within the 1e-6 bar of the launch-form tests (m3500_inc_demo.npz) -- the checker rejects it at
    once.  The gap, kept as a measurement."""
    G = golden("m3500_inc_demo.npz")
    n = 420
    chk = IncExact(reflib, oracle, model_lib=lib, strict=False, after_call=_offset(lambda w: np.nonzero(w)[0], 1e-6, 250))
    res = harness.run_demo(chk, datasets.m3500_arrays(), max_poses=n)
    rel = float(np.max(np.abs(res["chi2"] - G["chi2"][:n]) / np.maximum(G["chi2"][:n], 1e-9)))
    r = chk.report
    print(f"1e-6 offsets from step 250: chi^2 trace relative error {rel:.2e} (bar 1e-6); checker {r['inc_state']:.2e}, "
          f"{r['failures']} of {r['checked']} steps rejected")
    assert rel < 1e-6                                      # the trace bar does not see it ...
    assert r["inc_state"] > 0.9e-6 and r["failures"] >= n - 250 - len(r["fallback_nodes"]) - 1     # ... the checker rejects every such step
