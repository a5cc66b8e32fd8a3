"""Levenberg-Marquardt without a GPU: the numpy model's identities and runs, the ABI of the new structs, and the
loud refusal on a machine without a HIP device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from aprilsam_amd import abi, datasets
from tests.support import lm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def m3500():
    st, fa, fb, z, W = datasets.m3500_batch()
    return st, (fa, fb, z, W)


def _pred_vs_identity(x, plain, lam):
    fa, fb, z, W = plain
    A0, B = M.system(x, fa, fb, z, W, 0.0)
    A, _ = M.system(x, fa, fb, z, W, lam)
    import scipy.sparse.linalg as spla
    h = spla.spsolve(A, B)
    pred = float(np.sum(M.pred_terms(x, h, fa, fb, z, W)))
    ident = float(h @ B + lam * (h @ h))
    return pred, ident


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pred_equals_hB_plus_lambda_h2_random(seed):
    st, fa, fb, z, W = datasets.random_pose_graph(60, 40, seed)
    for lam in (1e-4, 1e-1, 10.0):
        pred, ident = _pred_vs_identity(M.perturbed(st, 0.5, seed), (fa, fb, z, W), lam)
        assert abs(pred - ident) <= 1e-10 * abs(ident), (lam, pred, ident)


def test_pred_equals_hB_plus_lambda_h2_m3500(m3500):
    st, plain = m3500
    for sigma, lam in ((0.3, 1e-4), (1.0, 1e-2)):
        pred, ident = _pred_vs_identity(M.perturbed(st, sigma), plain, lam)
        assert abs(pred - ident) <= 1e-10 * abs(ident), (sigma, pred, ident)


def test_converged_starts_stop_on_ftol(m3500):
    st, plain = m3500
    F_gn, _ = M.gn_steps(st, plain, 10, lam=0.0)
    for x0 in (st, M.perturbed(st, 0.3)):
        r = M.optimize(x0, plain)
        assert r["status"] == M.CONVERGED_F and r["iterations"] <= 12, (r["status"], r["iterations"])
        assert abs(r["F_final"] - F_gn[-1]) <= 1e-9 * F_gn[-1], (r["F_final"], F_gn[-1])
        assert abs(r["F_final"] - 137.913) < 1e-3


def test_divergent_start_monotone(m3500):
    st, plain = m3500
    x0 = M.perturbed(st, 1.0)
    F_gn, _ = M.gn_steps(x0, plain, 20, lam=0.0)
    assert F_gn[-1] > 1e7, F_gn
    r = M.optimize(x0, plain, max_iters=60)
    acc = r["trace"][r["trace"][:, 3] == 1, 0]
    assert np.all(np.diff(np.concatenate([[r["F_initial"]], acc])) < 0)
    assert r["F_final"] < 5e4 and r["iterations"] <= 60


def test_latch_makes_runs_prefixes(m3500):
    """a run cut at k iterations is the first k rows of a longer run (what check_every relies on)"""
    st, plain = m3500
    x0 = M.perturbed(st, 1.0)
    a = M.optimize(x0, plain, max_iters=6); b = M.optimize(x0, plain, max_iters=10)
    assert a["status"] == M.MAX_ITERS and a["iterations"] == 6
    assert np.array_equal(a["trace"], b["trace"][:6])


def test_lm_structs_match_header(tmp_path, built):
    src = tmp_path / "lm_abi.c"
    src.write_text("""#include <stdio.h>
#include <stddef.h>
#include "aprilsam_amd.h"
#define O(T, f) printf(#T " " #f " %zu\\n", offsetof(T, f))
int main(void) {
    printf("sizes %zu %zu\\n", sizeof(aprilsam_amd_lm_opts_t), sizeof(aprilsam_amd_lm_report_t));
    O(aprilsam_amd_lm_opts_t, max_iters); O(aprilsam_amd_lm_opts_t, check_every); O(aprilsam_amd_lm_opts_t, lambda0);
    O(aprilsam_amd_lm_opts_t, lambda_max); O(aprilsam_amd_lm_opts_t, eta); O(aprilsam_amd_lm_opts_t, ftol); O(aprilsam_amd_lm_opts_t, xtol);
    O(aprilsam_amd_lm_report_t, status); O(aprilsam_amd_lm_report_t, iterations); O(aprilsam_amd_lm_report_t, accepted);
    O(aprilsam_amd_lm_report_t, rejected_not_spd); O(aprilsam_amd_lm_report_t, F_initial); O(aprilsam_amd_lm_report_t, F_final);
    O(aprilsam_amd_lm_report_t, chi2_final); O(aprilsam_amd_lm_report_t, lambda_final);
    printf("status %d %d %d %d\\n", APRILSAM_AMD_LM_CONVERGED_F, APRILSAM_AMD_LM_CONVERGED_X, APRILSAM_AMD_LM_STALLED, APRILSAM_AMD_LM_MAX_ITERS);
    return 0;
}
""")
    exe = tmp_path / "lm_abi"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert out[0] == f"sizes {C.sizeof(abi.LmOpts)} {C.sizeof(abi.LmReport)}"
    for line in out[1:-1]:
        T, f, off = line.split()
        cls = abi.LmOpts if T == "aprilsam_amd_lm_opts_t" else abi.LmReport
        assert getattr(cls, f).offset == int(off), line
    assert out[-1] == f"status {abi.LM_CONVERGED_F} {abi.LM_CONVERGED_X} {abi.LM_STALLED} {abi.LM_MAX_ITERS}"


def test_lm_opts_init_defaults(lib):
    o = abi.LmOpts()
    lib.dll.aprilsam_amd_lm_opts_init(C.byref(o))
    assert (o.max_iters, o.check_every, o.lambda0, o.lambda_max, o.eta, o.ftol, o.xtol) == (50, 1, 1e-4, 1e16, 0.0, 1e-10, 1e-10)


def test_optimize_lm_fails_loudly_without_gpu(lib):
    if lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from aprilsam_amd import host, datasets\n"
            "l = host.SolverLib(); g = l.new_graph(); g.build_from_arrays(*datasets.random_pose_graph(5, 2, 0))\n"
            "before = (g.states().copy(), g.l_points().copy(), g.deltas().copy())\n"
            "p = l.new_param()\n"
            "try:\n"
            "    g.optimize_lm(p); raise SystemExit('no error raised')\n"
            "except host.LMError as e:\n"
            "    assert e.code == -14, e.code\n"
            "rc, msg = l.last_error()\n"
            "assert rc == -14 and 'no HIP device' in msg, (rc, msg)\n"
            "assert all((a == b).all() for a, b in zip(before, (g.states(), g.l_points(), g.deltas()))), 'graph was touched'\n"
            "print('RETURNED')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RETURNED" in r.stdout, (r.stdout, r.stderr)
    assert "no HIP device" in r.stderr


def test_optimize_lm_refuses_bad_options_without_touching_the_graph(lib):
    from aprilsam_amd import host
    g = lib.new_graph(); g.build_from_arrays(*datasets.random_pose_graph(5, 2, 0)); p = lib.new_param()
    before = g.states().copy()
    for bad in (dict(max_iters=0), dict(check_every=0), dict(lambda0=0.0), dict(lambda0=float("nan")), dict(eta=1.0), dict(ftol=-1.0),
                dict(xtol=float("inf")), dict(lambda_max=-1.0)):
        with pytest.raises(host.LMError) as e:
            g.optimize_lm(p, **bad)
        assert e.value.code == -13, bad
        assert lib.last_error()[0] == -13
    assert (g.states() == before).all()
    p.destroy(); g.destroy()


def test_rejection_of_a_step_whose_system_is_not_positive_definite(lib):
    """the chain with one prior of negative information (tests/support/pivot_placement.py): the model rejects exactly the iterations whose
    sum J'WJ + lambda I has a negative eigenvalue, counts them, multiplies lambda by nu and doubles nu, as k_lm_decide does; every decision
    stays clear of rounding; and on a positive definite graph the check changes nothing"""
    from tests.support import pivot_placement as pp
    prm = lib.new_param(); lam0 = float(prm.c.tikhanov); prm.destroy()
    pl = pp.placement(lib, "chain", 16, lam0)
    seqs = []
    for k, delta in pp.LM_CASES:
        st, fa, fb, z, W = pl.case(*pl.classes()[k], delta=delta)["arr"]
        r = M.optimize(st, (fa, fb, z, W), max_iters=pp.LM_ITERS, spd_check=pp.ldl_pivots)
        t = r["trace"]
        assert r["iterations"] == pp.LM_ITERS and r["margins"].min() > pp.LM_MARGIN
        nspd = np.isnan(t[:, 0])
        assert nspd[0] and r["rejected_not_spd"] == int(nspd.sum()) >= 4 and r["accepted"] == int(t[:, 3].sum()) >= 4
        assert not np.any(nspd & (t[:, 3] == 1))
        lam, nu = 1e-4, 2.0
        x = np.array(st, float)
        for i in range(len(t)):
            assert t[i, 2] == lam
            A, _ = M.system(x, fa, fb, z, W, lam)
            assert (np.linalg.eigvalsh(A.toarray())[0] <= 0) == bool(nspd[i]), (k, i)
            if t[i, 3] == 1:
                u = 2.0 * t[i, 1] - 1.0
                lam, nu = lam * max(1.0 / 3.0, 1.0 - u * u * u), 2.0
            else:
                lam, nu = lam * nu, 2.0 * nu
            x = r["xs"][i]
        assert r["lambda_final"] == lam
        seqs.append("".join("N" if a else ("A" if b else "r") for a, b in zip(nspd, t[:, 3] == 1)))
    assert seqs == ["NNNNAAAArAArrArr", "NNNNNNNAAAAANNAr", "NNNNNNANANNAANNA"], seqs
    st, fa, fb, z, W = pp.graph("chain")
    a = M.optimize(st, (fa, fb, z, W), max_iters=6, spd_check=pp.ldl_pivots); b = M.optimize(st, (fa, fb, z, W), max_iters=6)
    assert a["rejected_not_spd"] == 0 and a["trace"].tobytes() == b["trace"].tobytes() and a["x"].tobytes() == b["x"].tobytes()
