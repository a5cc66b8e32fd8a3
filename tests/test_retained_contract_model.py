"""The retained-factor contract table and the logic that judges it, without a GPU (tests/support/retained_contract.py).

* the table is complete: every event has every consumer, every value is a System the events record or a code the header lists for that
  entry point;
* discrimination -- a condition on the scene, not a measurement of the library: for every event that names a new System the REPLACED
  System's reference output fails the same checker against the new System by at least 1000 times its tolerance, and for the events that
  only move the states the same holds for the two consumers that read them.  The events are restated with numpy Gauss-Newton steps;
* negative controls of judge(), the function the GPU test decides every cell with, on fabricated answers: the previous system's numbers
  where the table names the new one, 0 where it names a refusal, a refusal that wrote one output element."""
import numpy as np
import pytest

from tests.support import retained_contract as rc

# consumers whose answer cannot tell two systems of the same size apart (the node count), kept out of the discrimination condition
SAME_ANSWER = {c.name for c in rc.CONSUMERS if not c.discriminates}


def test_the_table_is_complete():
    names = [c.name for c in rc.CONSUMERS]
    assert len(names) == 13 and len(set(names)) == 13
    assert set(rc.EXPECTED) == set(rc.EVENTS)
    for order in rc.ORDERS.values():
        assert sorted(order) == sorted(names)
    for ev, row in rc.EXPECTED.items():
        assert set(row) == set(names), ev
        for name, v in row.items():
            assert v in rc.SYSTEM_NAMES or v in rc.CODES[name], (ev, name, v)
            if name in rc.INC:
                assert v in rc.CODES[name], (ev, name, v)          # (the void entry points never name a System: see Incremental)
    # every System the table names is one an event records (S0: the two calls before every event)
    named = {v for row in rc.EXPECTED.values() for v in row.values() if v in rc.SYSTEM_NAMES}
    assert named == rc.SYSTEM_NAMES
    md = rc.table_markdown()
    assert md.count("\n") == len(rc.EXPECTED) + 1
    # the families scene: every event has the thirteen consumers and the four of its own
    fam_names = names + rc.FAM
    assert len(rc.FAM) == 4 and set(rc.EXPECTED_FAM) == set(rc.FAM_EVENTS) and sorted(rc.FAM_ORDER) == sorted(fam_names)
    assert {"32_robust_scale", "33_mixture_z", "34_polar_z", "35_gaussian_eta"} <= set(rc.FAM_EVENTS) and len(rc.FAM_NEW_SYSTEM_EVENTS) == 4
    for ev, row in rc.EXPECTED_FAM.items():
        assert set(row) == set(fam_names), ev
        for name, v in row.items():
            assert v in ("S0", "S1") or v in rc.CODES[name], (ev, name, v)


def test_design_section_25_holds_the_table_as_built():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    assert "## 25. What ends a retained factor" in text
    for line in rc.table_markdown().splitlines() + rc.table_markdown(families=True).splitlines():
        assert line in text, line


def test_the_table_quotes_the_header():
    """every phrase a row of EXPECTED quotes stands in include/aprilsam_amd.h (whitespace and the comment's line starts apart)"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    norm = lambda t: re.sub(r"\s+", " ", re.sub(r"\n\s*\*\s?", " ", t))
    header = norm(open(os.path.join(root, "include", "aprilsam_amd.h")).read())
    src = open(os.path.join(root, "tests", "support", "retained_contract.py")).read()
    block = src[src.index("EXPECTED = {"):src.index("CODES = {c:")]
    comments = norm(" ".join(line.strip().lstrip("#") for line in block.splitlines() if line.strip().startswith("#")))
    quotes = [q for q in re.findall(r'"([^"]+)"', comments)]
    pieces = [p.strip() for q in quotes for p in q.split(" ... ") if len(p.strip()) > 12]
    assert len(pieces) > 25
    missing = [p for p in pieces if p not in header]
    assert not missing, missing


@pytest.mark.parametrize("event", rc.NEW_SYSTEM_EVENTS + rc.STATE_EVENTS)
def test_the_replaced_system_fails_every_checker_by_a_factor_of_1000(event):
    d = rc.discrimination(event)
    print(f"[retained contract] discrimination {event}: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items()))
    want = ["gate_xyt", "relative_covariances"] if event in rc.STATE_EVENTS else \
        [n for n in rc.POOL + rc.LIN if rc.EXPECTED[event][n] in rc.SYSTEM_NAMES]
    assert set(want) <= set(d), (event, sorted(set(want) - set(d)))
    for name in want:
        assert d[name] >= rc.DISCRIMINATION, (event, name, d[name])


@pytest.mark.parametrize("event", rc.FAM_NEW_SYSTEM_EVENTS)
def test_the_replaced_families_system_fails_every_checker_by_a_factor_of_1000(event):
    d = rc.fam_discrimination(event)
    print(f"[retained contract] discrimination {event}: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items()))
    for name, v in d.items():
        if rc.BY_NAME[name].discriminates:
            assert v >= rc.DISCRIMINATION, (event, name, v)
    if "mixture" in event:                       # the edit flips the selection: here even the index tells the systems apart
        assert d["max_selected"] >= rc.DISCRIMINATION


def test_a_families_system_passes_its_own_checkers():
    old, new, x_old, x_new = rc.fam_shadow("36b_mixture_z_solved")
    assert old.info["sel"] == 0 and new.info["sel"] == 1 and 0 < old.info["w"] < 1
    for name in rc.POOL + rc.LIN + rc.FAM + ["factorised_nodes"]:
        cons = rc.BY_NAME[name]
        assert cons.ratio(cons.model(new, x_new), new, x_new) < 1.0, name
        cons.check(cons.model(new, x_new), new, x_new)
        assert cons.untouched(cons.blank(new, x_new)), name


def test_a_system_passes_its_own_checkers():
    """the positive control of the condition above: every reference output is within tolerance of its own System"""
    old, new, x_old, x_new = rc.shadow("03_third_call")
    for cons in rc.CONSUMERS:
        if cons.name in rc.INC:
            continue
        assert cons.ratio(cons.model(new, x_new), new, x_new) < 1.0, cons.name
        cons.check(cons.model(new, x_new), new, x_new)


# ---- negative controls of judge() -------------------------------------------------------------------------------------------------
class FakeLib:
    """answers in place of the library: `behaviour` says how it misbehaves"""

    def __init__(self, behaviour, old, new, x_old, x_new):
        self.behaviour, self.old, self.new, self.x_old, self.x_new = behaviour, old, new, x_old, x_new

    def answer(self, cons):
        """-> (rc, outputs, aprilsam_amd_last_error)"""
        if self.behaviour == "honest":
            return 0, cons.model(self.new, self.x_new), 0
        if self.behaviour == "stale":                                # the previous system's correct numbers
            return 0, cons.model(self.old, self.x_new), 0
        if self.behaviour == "honest_refusal":
            return -1, cons.blank(self.new, self.x_new), -1
        if self.behaviour == "answers_where_it_must_refuse":
            return 0, cons.model(self.new, self.x_new), 0
        if self.behaviour == "refusal_that_writes":
            out = cons.blank(self.new, self.x_new)
            k = sorted(out)[0]
            out[k].reshape(-1)[-1] = 0.125
            return -1, out, -1
        raise ValueError(self.behaviour)


@pytest.fixture(scope="module")
def systems():
    old, new, x_old, x_new = rc.shadow("03_third_call")
    old.name, new.name = "S0", "S1"
    return old, new, x_old, x_new


FP = dict(plan=(41, 44), selinv_runs=1, states=b"s", l_points=b"l", delta_X=b"d")
JUDGED = [c for c in rc.CONSUMERS if c.name not in rc.INC]


def _judge(fake, cons, expected, fp_after=FP):
    rc_, out, err = fake.answer(cons)
    S = {"S0": fake.old, "S1": fake.new}
    return rc.judge(cons, expected, rc_, out, S, fake.x_new, err, FP, fp_after, replaced=fake.old if expected == "S1" else None)[0]


@pytest.mark.parametrize("cons", JUDGED, ids=lambda c: c.name)
def test_judge_accepts_the_right_answer_and_a_clean_refusal(systems, cons):
    assert _judge(FakeLib("honest", *systems), cons, "S1") == []
    assert _judge(FakeLib("honest_refusal", *systems), cons, -1) == []


@pytest.mark.parametrize("cons", [c for c in JUDGED if c.name not in SAME_ANSWER], ids=lambda c: c.name)
def test_judge_reports_the_previous_system_s_numbers(systems, cons):
    bad = _judge(FakeLib("stale", *systems), cons, "S1")
    assert any("does not answer for S1" in b for b in bad), bad
    assert any("answers for the replaced system S0" in b for b in bad), bad


@pytest.mark.parametrize("cons", JUDGED, ids=lambda c: c.name)
def test_judge_reports_an_answer_where_the_table_names_a_refusal(systems, cons):
    bad = _judge(FakeLib("answers_where_it_must_refuse", *systems), cons, -1)
    assert any("where the table says -1" in b for b in bad), bad


@pytest.mark.parametrize("cons", JUDGED, ids=lambda c: c.name)
def test_judge_reports_a_refusal_that_writes_one_element(systems, cons):
    bad = _judge(FakeLib("refusal_that_writes", *systems), cons, -1)
    assert any("wrote into its outputs" in b for b in bad), bad


def test_judge_reports_a_refusal_that_costs_something(systems):
    cons = rc.BY_NAME["marginals_all"]
    for key, val in (("selinv_runs", 2), ("states", b"x"), ("plan", (41, 45))):
        bad = _judge(FakeLib("honest_refusal", *systems), cons, -1, dict(FP, **{key: val}))
        assert any(key in b for b in bad), (key, bad)
    rc_, out, _ = FakeLib("honest_refusal", *systems).answer(cons)
    bad = rc.judge(cons, -1, rc_, out, {}, systems[3], 0, FP, FP)[0]       # the code returned but not recorded
    assert any("aprilsam_amd_last_error" in b for b in bad), bad


def test_judge_on_the_void_incremental_entry_points(systems):
    cons = rc.BY_NAME["cholesky_inc"]
    same, written = dict(same=np.array([rc.SENT])), dict(same=np.array([1.0]))
    assert rc.judge(cons, "noop", 0, same, {}, systems[3], 0, FP, FP)[0] == []
    assert rc.judge(cons, "noop", 0, written, {}, systems[3], 0, FP, FP)[0]
    assert rc.judge(cons, "noop", -12, same, {}, systems[3], -12, FP, FP)[0]
    assert rc.judge(cons, -12, -12, same, {}, systems[3], -12, FP, FP)[0] == []
    assert rc.judge(cons, -12, 0, same, {}, systems[3], 0, FP, FP)[0]
    assert rc.judge(cons, -12, -12, written, {}, systems[3], -12, FP, FP)[0]
