"""Chordal initialisation without a GPU: the numpy model (tests/support/chordal_model.py) pinned by exact recovery,
by what it buys LM on M3500, by the padded 3-unknown form and by its own spread over orderings; the ABI of the new structs; the loud
refusal on a machine without a HIP device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from aprilsam_amd import abi, datasets
from tests.support import chordal_model as CM
from tests.support import lm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def m3500():
    st, fa, fb, z, W = datasets.m3500_batch()
    return st, (fa, fb, z, W)


@pytest.fixture(scope="module")
def m3500_chordal(m3500):
    st, plain = m3500
    return CM.initialize(plain, np.zeros_like(st))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_exact_measurements_are_recovered(seed):
    st, fa, fb, z, W = datasets.random_pose_graph(300, 200, seed)
    plain = (fa, fb, CM.exact_measurements(st, fa, fb), W)
    r = CM.initialize(plain, np.zeros_like(st))
    print("exact recovery, seed", seed, CM.state_diff(r["x"], st))
    assert r["n_degenerate"] == 0 and abs(r["min_norm"] - 1.0) < 1e-9
    assert CM.state_diff(r["x"], st) < 1e-10
    out = CM.residuals(plain, r["u"], r["x"])
    assert out["rel1"] < 1e-10 and out["rel2"] < 1e-10, out


def test_m3500_cost_drops_a_thousandfold(m3500, m3500_chordal):
    st, plain = m3500
    Fc, Fg = M.cost(m3500_chordal["x"], plain), M.cost(st, plain)
    print("M3500: F(chordal)", Fc, "F(golden start)", Fg)
    assert Fc < 1e-3 * Fg


def test_m3500_lm_converges_from_the_chordal_start(m3500, m3500_chordal):
    st, plain = m3500
    r = M.optimize(m3500_chordal["x"], plain)
    print("M3500: LM from the chordal start", r["status"], r["iterations"], r["F_final"])
    assert r["status"] == M.CONVERGED_F and r["iterations"] <= 12
    assert abs(r["F_final"] - 137.913) <= 1e-6 * 137.913


def test_m3500_lm_from_zero_states_does_not(m3500):
    st, plain = m3500
    r = M.optimize(np.zeros_like(st), plain)
    print("M3500: LM from all-zero states", r["status"], r["iterations"], r["F_final"])
    assert r["status"] == M.MAX_ITERS and r["F_final"] > 1e4


@pytest.mark.parametrize("case", ["random0", "m3500"])
def test_padded_system_gives_the_same_answer(case, m3500):
    if case == "m3500":
        st, plain = m3500
    else:
        st, *plain = datasets.random_pose_graph(300, 200, 0)
    a = CM.initialize(plain, np.zeros_like(st)); b = CM.initialize(plain, np.zeros_like(st), pad=True)
    assert np.all(b["pad1"] == 0) and np.all(b["pad2"] == 0)
    # (the padding changes the elimination order COLAMD finds, not the system: the model's own spread bounds the difference)
    assert CM.state_diff(a["x"], b["x"]) <= max(1e-12, 10 * CM.spread(plain, np.zeros_like(st)))


def test_the_models_own_spread(lib, m3500):
    """s_case of every graph tests/test_gpu_chordal.py uses, recorded in profiles/chordal_model_spread.txt"""
    st, plain = m3500
    rows = [("m3500", CM.spread(plain, np.zeros_like(st)))]
    for seed in range(4):
        st, *p = datasets.random_pose_graph(300, 200, seed)
        rows.append((f"random{seed}", CM.spread(p, np.zeros_like(st))))
    st, *p = lib.lattice_arrays(24)
    rows.append(("lattice24", CM.spread(p, np.zeros_like(st))))
    text = "# largest state difference of tests/support/chordal_model.py between permc_spec COLAMD, NATURAL and MMD_AT_PLUS_A\n"
    text += "".join(f"{n:10s} {s:.3e}\n" for n, s in rows)
    print(text)
    try:
        with open(os.path.join(ROOT, "profiles", "chordal_model_spread.txt"), "w") as f:
            f.write(text)
    except OSError:
        pass                        # (a read-only checkout: the record is not the check)
    assert all(np.isfinite(s) for _, s in rows), rows


def test_without_a_heading_prior_stage_1_says_nothing():
    """why the refusal is structural: with noisy loops the stage-1 matrix of a graph without a heading prior is not even singular, and
    its solution is u = 0 on every pose"""
    st, fa, fb, z, W = datasets.random_pose_graph(20, 5, 0)
    W = np.array(W, float).reshape(-1, 9); W[fb < 0, 8] = 0
    plain = (fa, fb, z, W)
    A, B = CM.stage1_system(len(st), plain)
    assert not B.any()
    assert CM.unanchored_stage(plain, len(st)) == 1
    r = CM.initialize(plain, st, stages=1)
    assert r["n_degenerate"] == len(st) and np.array_equal(r["x"], st)
    # a heading-only prior anchors stage 1 and leaves stage 2 adrift; an xy-only prior elsewhere anchors that too
    W[fb < 0] = np.diag([0.0, 0.0, 10.0]).reshape(9)
    assert CM.unanchored_stage(plain, len(st)) == 2 and CM.unanchored_stage(plain, len(st), stages=1) == 0
    fa2 = np.append(fa, 7); fb2 = np.append(fb, -1); z2 = np.vstack([z, [1.0, 2.0, 0.0]]); W2 = np.vstack([W, np.diag([5.0, 5.0, 0.0]).reshape(9)])
    assert CM.unanchored_stage((fa2, fb2, z2, W2), len(st)) == 0


def test_chordal_structs_match_header(tmp_path, built):
    src = tmp_path / "chordal_abi.c"
    src.write_text("""#include <stdio.h>
#include <stddef.h>
#include "aprilsam_amd.h"
#define O(T, f) printf(#T " " #f " %zu\\n", offsetof(T, f))
int main(void) {
    printf("sizes %zu %zu\\n", sizeof(aprilsam_amd_chordal_opts_t), sizeof(aprilsam_amd_chordal_report_t));
    O(aprilsam_amd_chordal_opts_t, stages);
    O(aprilsam_amd_chordal_report_t, status); O(aprilsam_amd_chordal_report_t, n_degenerate); O(aprilsam_amd_chordal_report_t, not_spd_stage);
    O(aprilsam_amd_chordal_report_t, min_norm); O(aprilsam_amd_chordal_report_t, F_initial); O(aprilsam_amd_chordal_report_t, F_final);
    return 0;
}
""")
    exe = tmp_path / "chordal_abi"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert out[0] == f"sizes {C.sizeof(abi.ChordalOpts)} {C.sizeof(abi.ChordalReport)}"
    for line in out[1:]:
        T, f, off = line.split()
        cls = abi.ChordalOpts if T == "aprilsam_amd_chordal_opts_t" else abi.ChordalReport
        assert getattr(cls, f).offset == int(off), line


def test_chordal_symbols_and_defaults(lib):
    assert hasattr(lib.dll, "aprilsam_amd_initialize_chordal") and hasattr(lib.dll, "aprilsam_amd_chordal_opts_init")
    o = abi.ChordalOpts()
    lib.dll.aprilsam_amd_chordal_opts_init(C.byref(o))
    assert o.stages == 3


def test_initialize_chordal_fails_loudly_without_gpu(lib):
    if lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from aprilsam_amd import host, datasets\n"
            "l = host.SolverLib(); g = l.new_graph(); g.build_from_arrays(*datasets.random_pose_graph(5, 2, 0))\n"
            "before = (g.states().copy(), g.l_points().copy(), g.deltas().copy())\n"
            "p = l.new_param()\n"
            "try:\n"
            "    g.initialize_chordal(p); raise SystemExit('no error raised')\n"
            "except host.ChordalError as e:\n"
            "    assert e.code == -14, e.code\n"
            "rc, msg = l.last_error()\n"
            "assert rc == -14 and 'no HIP device' in msg, (rc, msg)\n"
            "assert all((a == b).all() for a, b in zip(before, (g.states(), g.l_points(), g.deltas()))), 'graph was touched'\n"
            "print('RETURNED')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RETURNED" in r.stdout, (r.stdout, r.stderr)
    assert "no HIP device" in r.stderr


def test_initialize_chordal_refuses_bad_arguments_without_touching_the_graph(lib):
    from aprilsam_amd import host
    g = lib.new_graph(); g.build_from_arrays(*datasets.random_pose_graph(5, 2, 0)); p = lib.new_param()
    before = g.states().copy()
    for bad in (dict(stages=0), dict(stages=2), dict(stages=4)):
        with pytest.raises(host.ChordalError) as e:
            g.initialize_chordal(p, **bad)
        assert e.value.code == -13 and lib.last_error()[0] == -13, bad
    with pytest.raises(host.ChordalError) as e:
        g.initialize_chordal(None)
    assert e.value.code == -13
    ge = lib.new_graph()
    with pytest.raises(host.ChordalError) as e:
        ge.initialize_chordal(p)
    assert e.value.code == -1
    assert (g.states() == before).all()
    p.destroy(); g.destroy(); ge.destroy()
