"""Graduated non-convexity without a GPU: the surrogate formulas of the numpy model, the model's runs on the snake
scenarios, the ABI of the new structs, and the refusals that need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from aprilsam_amd import abi, datasets
from tests.support import gnc_model as G
from tests.support import lm_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = [G.GM, G.TLS]
MUS = [1e-4, 0.03, 1.0, 7.5, 3e4]


@pytest.mark.parametrize("mu", MUS)
def test_tls_surrogate_is_continuous_at_lo_and_hi(mu):
    c = G.C_DEFAULT
    for edge in G._bounds(c, mu):
        below, above = edge * (1 - 1e-9), edge * (1 + 1e-9)
        # (rho has slope <= 1 and w slope <= (mu + 1) / (2 lo) there: a step of 1e-9 edge moves neither by more than 1e-6 of its scale)
        assert abs(G.rho(G.TLS, c, mu, below) - G.rho(G.TLS, c, mu, above)) <= 1e-8 * edge
        assert abs(G.weight(G.TLS, c, mu, below) - G.weight(G.TLS, c, mu, above)) <= 1e-6 * (1 + mu)
    lo, hi = G._bounds(c, mu)
    assert G.weight(G.TLS, c, mu, lo) == 1.0 and G.weight(G.TLS, c, mu, hi) == 0.0
    assert G.rho(G.TLS, c, mu, lo) == lo and G.rho(G.TLS, c, mu, hi) == c * c


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("mu", MUS)
def test_weight_is_the_derivative_of_rho(loss, mu):
    c = 2.5
    lo, hi = G._bounds(c, mu)
    pts = np.concatenate([np.geomspace(1e-3, 1e4, 40), np.linspace(lo, hi, 7)[1:-1]])
    for s in pts:
        d = 1e-6 * s
        if loss == G.TLS and (abs(s - lo) <= 2 * d or abs(s - hi) <= 2 * d):      # (the kinks of w)
            continue
        num = (G.rho(loss, c, mu, s + d) - G.rho(loss, c, mu, s - d)) / (2 * d)
        w = float(G.weight(loss, c, mu, s))
        # truncation d^2 / 6 times the third derivative of rho stays below 1e-9; TLS between lo and hi cancels terms of size mu (cc + s),
        # whose rounding 1e-16 mu (cc + s) over 2 d = 2e-6 s is 1e-10 mu (1 + cc / s), with s near cc there
        assert abs(num - w) <= 1e-6 + 1e-9 * mu, (loss, mu, s, num, w)


def test_limits_and_nan():
    c = 3.0
    s = np.array([0.0, 1.0, 8.9, 9.0, 9.1, 1e3])
    assert np.array_equal(G.weight(G.TLS, c, float("inf"), s), [1, 1, 1, 1, 0, 0])
    assert np.array_equal(G.rho(G.TLS, c, float("inf"), s), [0, 1, 8.9, 9, 9, 9])
    assert np.allclose(G.weight(G.GM, c, 1e12, s), 1.0, atol=1e-8) and np.allclose(G.rho(G.GM, c, 1e12, s), s, rtol=1e-8)
    for loss in LOSSES:
        for mu in (0.5, 1.0, float("inf")):
            assert np.isnan(G.weight(loss, c, mu, np.nan)) and np.isnan(G.rho(loss, c, mu, np.nan))
    assert G.mu_start(G.GM, c, 1.0) == (1.0, False) and G.mu_start(G.GM, c, 90.0) == (20.0, False)
    assert G.mu_start(G.TLS, c, 4.5) == (float("inf"), True) and G.mu_start(G.TLS, c, 9.0) == (1.0, False)


@pytest.mark.parametrize("case", G.CASES, ids=str)
@pytest.mark.parametrize("loss", LOSSES, ids=["GM", "TLS"])
def test_model_rejects_every_false_closure(case, loss):
    """the scenario generator was written from the issue's description alone; it separates on all three cases as given"""
    sc = G.snake(*case)
    r = G.model_run(case, loss)
    assert r["status"] == G.FINISHED and r["stages"] <= 40, (r["status"], r["stages"])
    inl = r["s"] <= G.C_DEFAULT ** 2
    assert not inl[sc["is_false"]].any() and inl[~sc["is_false"]].all()
    assert r["n_inliers"] == int((~sc["is_false"]).sum())
    if loss == G.GM:
        assert r["mu_final"] == 1.0 and r["weights"][sc["is_false"]].max() < 1e-6
    else:
        assert np.array_equal(r["weights"], (~sc["is_false"]).astype(float))
    plain = lm_model.optimize(sc["start"], sc["plain"])
    e_lm, e = G.position_error(plain["x"], sc["truth"]), G.position_error(r["x"], sc["truth"])
    assert e < 0.1 * e_lm, (e, e_lm)
    tr = r["stage_trace"]
    assert len(tr) == r["stages"] and tr[0, 0] == r["mu_initial"] and tr[-1, 0] == r["mu_final"] and tr[:, 3].sum() == r["iterations"]
    assert np.all(tr[:, 2] <= tr[:, 1])            # (a stage never ends above its entry objective)
    step = tr[1:, 0] / tr[:-1, 0]
    assert np.all(step < 1) if loss == G.GM else np.allclose(step, 1.4, rtol=1e-15)


def test_all_inlier_start_is_one_tls_stage():
    sc = G.snake(4, 0, 3)
    x = lm_model.optimize(sc["start"], sc["plain"])["x"]
    r = G.optimize(x, sc["plain"], sc["cand"], G.TLS)
    assert r["status"] == G.FINISHED and r["stages"] == 1 and np.isinf(r["mu_initial"]) and np.all(r["weights"] == 1.0)


def test_max_stages_ends_the_schedule():
    sc = G.snake(4, 3, 3)
    r = G.optimize(sc["start"], sc["plain"], sc["cand"], G.GM, max_stages=3)
    full = G.model_run((4, 3, 3), G.GM)
    assert r["status"] == G.MAX_STAGES and r["stages"] == 3 and np.array_equal(r["stage_trace"], full["stage_trace"][:3])


# ---- the ABI and the refusals that need no device --------------------------------------------------------------------------------------
def test_gnc_structs_match_header(tmp_path, built):
    fo = [f for f, _ in abi.GncOpts._fields_]; fr = [f for f, _ in abi.GncReport._fields_]
    lines = "".join(f"    O(aprilsam_amd_gnc_opts_t, {f});\n" for f in fo) + "".join(f"    O(aprilsam_amd_gnc_report_t, {f});\n" for f in fr)
    src = tmp_path / "gnc_abi.c"
    src.write_text("""#include <stdio.h>
#include <stddef.h>
#include "aprilsam_amd.h"
#define O(T, f) printf(#T " " #f " %zu\\n", offsetof(T, f))
int main(void) {
    printf("sizes %zu %zu\\n", sizeof(aprilsam_amd_gnc_opts_t), sizeof(aprilsam_amd_gnc_report_t));
""" + lines + """    printf("enums %d %d\\n", APRILSAM_AMD_GNC_GM, APRILSAM_AMD_GNC_TLS);
    return 0;
}
""")
    exe = tmp_path / "gnc_abi"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert out[0] == f"sizes {C.sizeof(abi.GncOpts)} {C.sizeof(abi.GncReport)}"
    assert len(out) == 2 + len(fo) + len(fr)
    for line in out[1:-1]:
        T, f, off = line.split()
        cls = abi.GncOpts if T == "aprilsam_amd_gnc_opts_t" else abi.GncReport
        assert getattr(cls, f).offset == int(off), line
    assert out[-1] == f"enums {abi.GNC_GM} {abi.GNC_TLS}"


def test_gnc_symbols_and_defaults(lib):
    for name in ("aprilsam_amd_gnc_opts_init", "aprilsam_amd_optimize_gnc", "aprilsam_amd_debug_graph_captures"):
        assert hasattr(lib.dll, name), name
    o = abi.GncOpts()
    lib.dll.aprilsam_amd_gnc_opts_init(C.byref(o))
    assert (o.loss, o.c, o.mu_step, o.max_stages) == (abi.GNC_GM, np.sqrt(16.27), 1.4, 100)
    assert (o.lm.max_iters, o.lm.check_every, o.lm.lambda0, o.lm.lambda_max, o.lm.eta, o.lm.ftol, o.lm.xtol) == (10, 1, 1e-4, 1e16, 0.0, 1e-10, 1e-10)
    assert G.C_DEFAULT == o.c


def test_optimize_gnc_fails_loudly_without_gpu(lib):
    if lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from aprilsam_amd import host\n"
            "from tests.support import gnc_model as G\n"
            "sc = G.snake(4, 3, 3)\n"
            "l = host.SolverLib(); g = l.new_graph(); g.build_from_arrays(sc['start'], *sc['plain'])\n"
            "before = (g.states().copy(), g.l_points().copy(), g.deltas().copy())\n"
            "p = l.new_param()\n"
            "try:\n"
            "    g.optimize_gnc(p, sc['cand']); raise SystemExit('no error raised')\n"
            "except host.GncError as e:\n"
            "    assert e.code == -14, e.code\n"
            "rc, msg = l.last_error()\n"
            "assert rc == -14 and 'no HIP device' in msg, (rc, msg)\n"
            "assert all((a == b).all() for a, b in zip(before, (g.states(), g.l_points(), g.deltas()))), 'graph was touched'\n"
            "print('RETURNED')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RETURNED" in r.stdout, (r.stdout, r.stderr)
    assert "no HIP device" in r.stderr


def test_optimize_gnc_refuses_bad_arguments_without_touching_the_graph(lib):
    from aprilsam_amd import host
    sc = G.snake(4, 3, 3)
    g = lib.new_graph(); g.build_from_arrays(sc["start"], *sc["plain"]); p = lib.new_param()
    before = g.states().copy()
    cand = sc["cand"]

    def expect(code, cand=cand, **kw):
        with pytest.raises(host.GncError) as e:
            g.optimize_gnc(p, cand, **kw)
        assert e.value.code == code and lib.last_error()[0] == code, (e.value.code, kw)

    for bad in (dict(loss=0), dict(loss=3), dict(c=0.0), dict(c=float("inf")), dict(c=float("nan")), dict(mu_step=1.0), dict(mu_step=float("nan")),
                dict(max_stages=0), dict(max_iters=0), dict(check_every=0), dict(lambda0=0.0), dict(eta=1.0)):
        expect(-13, **bad)
    expect(-13, cand=[])
    expect(-13, cand=None)
    expect(-13, cand=[int(cand[0]), g.n_factors])
    expect(-13, cand=[-1])
    expect(-13, cand=[int(cand[0]), int(cand[1]), int(cand[0])])
    # candidates that cannot carry the surrogate: a factor with a loss of its own, a max factor, a W that is not positive definite
    assert g.set_robust(int(cand[0]), abi.ROBUST_CAUCHY, 2.0) == 0
    expect(-12, cand=cand)
    assert g.set_robust(int(cand[0]), abi.ROBUST_NONE) == 0
    W = np.diag([1.0, 1.0, 1.0]).reshape(9)
    m = g.add_factor_max(0, 5, [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [W, W], [0.0, -1.0])
    expect(-12, cand=[int(cand[0]), m])
    g.add_factor_xyt(0, 7, [1.0, 0.0, 0.0], np.diag([1.0, -1.0, 1.0]).reshape(9))
    expect(-12, cand=[g.n_factors - 1])
    assert (g.states() == before).all()
    ge = lib.new_graph()
    with pytest.raises(host.GncError) as e:
        ge.optimize_gnc(p, [0])
    assert e.value.code == -1
    for o in (p, g, ge):
        o.destroy()
