"""Incremental steps at every shape and limit of their kernels: the designed scenarios of tests/support/inc_designs.py (whose base plans and
claims tests/test_inc_designs.py pins on the CPU) through april_graph_cholesky_inc under the option sets that change the form a step takes.

Every call of every run is checked by tests/support/inc_exact.py (stride 1, strict) at the project's own bars: written states within 1e-9 of
l_point + x, delta_X within 1e-9 of x -- x the oracle's solution of the call's exact linear system --, written and visited sets those of the
restated bookkeeping, and every batch step with a normal-equation residual below 1e-10.  On top of that the run's largest deviations are held to
DX_FACTOR x INC_ORDER_DEV, INC_ORDER_DEV being what the oracle deviates from ITSELF over elimination orders on these very systems
(inc_designs.py); the factor of 100 is the one of tests/test_gpu_front_shapes.py, for the reason given there: the kernels associate sums
differently from any CPU order, every difference is of rounding size, and the bound still sits five orders of magnitude below 1e-9.

After every call the library's own record of what the step did (aprilsam_amd_debug_inc_forms) is held to what the scenario declares -- the rows
inc_designs.Model predicts: front, mode, nsb, nub, old_nub, mask, own factors, updated children and their update blocks, in place, mid -- and to
the path the option set leaves it; the classes the scenario claims are evaluated on the EXPORT's rows.  Without these a case can silently stop
reaching its branch.

inc_update = 0 re-assembles the fronts the default run updates: its states and delta_X agree with the default run's within the rounding-size
bar.  DESIGN.md promises no bitwise equality between option sets for incremental steps (pool_poison and use_graph are promised for batch and LM
steps only): nothing bitwise is asserted here.

Observed on an MI355X over all scenarios and option sets: |state - (lp + x)| <= 2.4e-15, |delta_X - x| <= 2.5e-15, batch residual <= 1.1e-15,
inc_update = 0 against the updated run <= 1.8e-15 (DESIGN.md section 30 has the figures per option set, the class table and the scratch
mutations these tests were seen to catch)."""
import numpy as np
import pytest

from tests.support import inc_designs as ID
from tests.support.inc_exact import IncExact
from tests.support.mf_emulator import PlanView

pytestmark = pytest.mark.gpu
DX_FACTOR = 100
DX_ATOL = DX_FACTOR * ID.INC_ORDER_DEV
OPTION_SETS = [dict(), dict(inc_update=0), dict(inc_one=0), dict(inc_multi=0), dict(inc_one_threads=256), dict(inc_one_threads=1024), dict(inc_inline=0), dict(pool_poison=1)]
TAIL_PATHS, GENERAL_PATHS = ("tail+solve", "tail+list", "tail general"), ("one", "multi", "levels")
FIELDS = ("front", "mode", "nsb", "nub", "old_nub", "mask", "n_own", "n_ch", "inplace", "mid", "ch_cnu")

_BUILT, _PLANS, _RUNS = {}, {}, {}


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _built(name):
    if name not in _BUILT:
        _BUILT[name] = ID.build(name)
    return _BUILT[name]


def _plan(lib, name):
    if name not in _PLANS:
        arr = ID.primed_arrays(_built(name))
        _PLANS[name] = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2])
    return _PLANS[name]


def _run(lib, oracle, name, opts):
    """the scenario under `opts`: per call the export, the states and delta_X it left; the IncExact report of the run"""
    key = (name, tuple(sorted(opts.items())))
    if key in _RUNS:
        return _RUNS[key]
    B, sc = _built(name), ID.SCENARIOS[name]
    chk = IncExact(lib, oracle, stride=1, strict=True, log=print)
    o = dict(opts)
    for k in ("tail_poses", "small_threads"):          # (what the scenario itself runs under)
        if sc[k]:
            o[k] = sc[k]
    calls = []
    with lib.options(**o):
        g = chk.new_graph(); g.build_from_arrays(*B["base"])
        p = lib.new_param(nthreshold=10 ** 6, delta_xy=ID.DELTA_XY, delta_theta=ID.DELTA_THETA)
        try:
            g.cholesky(p)
            for (st, fa, fb, z, W, ok) in B["calls"]:
                for s in st:
                    g.add_node_xyt(s)
                for a, b, zz, WW in zip(fa, fb, z, W):
                    if b >= 0:
                        g.add_factor_xyt(a, b, zz, WW.reshape(3, 3))
                    else:
                        g.add_factor_xytpos(a, zz, WW.reshape(3, 3))
                p.c.batch_time = 1e300                     # (the wall-clock rule of the reference never fires)
                g.cholesky_inc(p)
                stats = p.stats()
                assert stats["not_spd"] == 0 and stats["error_code"] == 0, (name, opts, len(calls), stats)
                head, rows = p.inc_forms()
                calls.append(dict(head=head, rows=rows, states=g.states(), deltas=g.deltas(), lp=g.l_points(), replanned=stats["inc_replanned"]))
        finally:
            p.destroy(); g.destroy()
    r = dict(calls=calls, report=chk.report)
    _RUNS[key] = r
    return r


def _export_rows(head, rows, declared):
    """the export's rows in the form the class predicates take (what the export does not carry -- the orientation of the own factors -- from
    the declaration of the same front)"""
    out = []
    for r, d in zip(rows, declared):
        e = dict(d)
        e.update({k: r[k] for k in FIELDS})
        e.update(ns=3 * r["nsb"], nu=3 * r["nub"], nu_o=3 * r["old_nub"], nact=ID.popcount(r["mask"]), nt=head["threads"])
        out.append(e)
    return out


def _check_forms(lib, name, opts, run):
    steps = ID.model_steps(name, _plan(lib, name), inc_update=opts.get("inc_update", 1), inc_multi=opts.get("inc_multi", 1))
    calls = run["calls"]
    assert len(calls) == len(steps) + 1
    h0 = calls[0]["head"]
    assert h0["path"] == "re-plan" and h0["fail"] == 3 and calls[0]["rows"] == [] and calls[0]["replanned"] == 1, (name, opts, h0)      # the primer
    for k, (step, call) in enumerate(zip(steps, calls[1:]), 1):
        head, rows = call["head"], call["rows"]
        what = (name, _ids(opts), f"call {k}", head, rows)
        print(f"FORM|{name}|{_ids(opts)}|call {k}|{head['path']} nt {head['threads']} one {head['one']} up {head['up_multi']} dn {head['dn_multi']} tail {head['a_idx']},{head['n_old']},{head['n_new']},{head['s_idx']}|"
              + " ".join(f"[{r['front']}{'U' if r['mode'] else 'A'} {r['nsb']} {r['old_nub']}->{r['nub']} m{r['mask']:b} o{r['n_own']} c{r['n_ch']}{r['ch_cnu']} ip{r['inplace']} mid{r['mid']}]" for r in rows))
        assert step[0] != "re-plan" and head["path"] != "re-plan" and call["replanned"] == 0, what
        S, declared = step
        assert head["n_factors"] == S["n_fac"], what
        assert [{f: r[f] for f in FIELDS} for r in rows] == [{f: d[f] for f in FIELDS} for d in declared], (what, declared)
        # the path: what the scenario declares (tail_refactor or not), what the option set leaves of it, what the step claims
        assert head["path"] in (TAIL_PATHS if S["tail_fast"] else GENERAL_PATHS), what
        if S["tail_fast"]:
            tail = [d for d in declared if d["last_tail"]][0]
            assert head["n_new"] == tail["nsb"] and head["n_new"] - head["a_idx"] == S["window"] and 0 <= head["a_idx"] <= head["n_old"] <= head["n_new"], what
            assert (head["s_idx"] >= 0) == (head["path"] == "tail+solve") and head["s_idx"] <= head["a_idx"], what
        else:
            assert head["a_idx"] == -1, what
        if opts.get("inc_one", 1) == 0:
            assert head["path"] in ("tail general", "multi", "levels") and head["one"] == 0, what
        if opts.get("inc_multi", 1) == 0:
            assert head["path"] == "levels" and head["up_multi"] == 0 and head["dn_multi"] == 0, what
        if head["one"]:
            assert head["threads"] == opts.get("inc_one_threads", ID.K["inc_one_threads"]), what
        if opts.get("inc_one_threads") == 1024:
            assert head["path"] != "tail+solve", what
        if opts.get("inc_update", 1) and opts.get("inc_multi", 1):        # (what the scenario is there for needs the updates and tail_refactor switched on)
            assert ID.claimed(name, k, S, _export_rows(head, rows, declared)) == [], what
        if opts == dict():
            for c in ID.SCENARIOS[name]["claims"].get(k, []):
                if c in ID.PATH_CLASSES:
                    assert head["path"] == ID.PATH_CLASSES[c], (c, what)
    if opts.get("inc_update", 1) and opts.get("inc_multi", 1):
        assert any(r["mode"] for c in calls for r in c["rows"]) == any(d["mode"] for s in steps for d in s[1])


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_ids)
@pytest.mark.parametrize("name", list(ID.SCENARIOS))
def test_every_designed_step_is_the_exact_solve_in_the_declared_form(lib, oracle, name, opts):
    run = _run(lib, oracle, name, opts)
    r = run["report"]
    print(f"FIGURE|{name}|{_ids(opts)}|state {r['inc_state']:.3e}|delta {r['inc_delta']:.3e}|batch residual {r['batch_res']:.3e}|calls {r['inc']}|near threshold {r['near_threshold']}")
    assert r["failures"] == 0 and r["inc"] == len(run["calls"]) and r["checked"] == r["inc"] and r["fallback"] == 0 and r["batch"] == 1, r
    assert r["near_threshold"] == 0, r                  # (no call whose written / visited sets went unchecked next to a relinearisation threshold)
    # no incremental call moves a linearisation point: the systems INC_ORDER_DEV was measured on (inc_designs.systems, l_points fixed) are this run's
    B = _built(name)
    lp0 = np.vstack([B["base"][0]] + [c[0] for c in B["calls"]])
    for k, call in enumerate(run["calls"]):
        assert np.array_equal(call["lp"], lp0[:len(call["lp"])]), (name, opts, k)
    _check_forms(lib, name, opts, run)
    assert r["inc_state"] <= DX_ATOL and r["inc_delta"] <= DX_ATOL, (name, opts, r["inc_state"], r["inc_delta"], DX_ATOL)
    if opts == dict(inc_update=0):                      # the same fronts re-assembled: the same numbers as the updated run, to rounding
        base = _run(lib, oracle, name, dict())
        dev = 0.0
        for a, b in zip(run["calls"], base["calls"]):
            e = a["states"] - b["states"]; e[:, 2] = (e[:, 2] + np.pi) % (2 * np.pi) - np.pi
            dev = max(dev, float(np.max(np.abs(e))), float(np.max(np.abs(a["deltas"] - b["deltas"]))))
        print(f"FIGURE|{name}|inc_update=0 against the updated run|{dev:.3e}")
        assert dev <= DX_ATOL, (name, dev)


def test_negative_control_a_row_of_the_export_off_by_one(lib, oracle):
    """the form assertion itself: one field of one row changed, and the comparison with the declaration fails"""
    name = next(iter(ID.SCENARIOS))
    run = _run(lib, oracle, name, dict())
    bent = dict(calls=[dict(c, rows=[dict(r) for r in c["rows"]]) for c in run["calls"]], report=run["report"])
    bent["calls"][1]["rows"][0]["old_nub"] += 1
    with pytest.raises(AssertionError):
        _check_forms(lib, name, dict(), bent)
