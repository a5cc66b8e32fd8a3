"""The not-positive-definite report and the recovery from it, on every factorisation form and every solve path.

tests/support/pivot_placement.py puts the FIRST non-positive pivot at a chosen scalar position of the elimination order (one prior with
W = -s e_d e_d' and residual 0 on one pose); the position classes come from the kernels' pivot checks (first column of a block, inside
a block, partial last block, every panel / outer-block position of k_block_chain, the last pivot of the last front).  What include/
aprilsam_amd.h promises for -2 is asserted per entry point: stats.not_spd, stats.error_code and aprilsam_amd_last_error, node states and
delta_X bitwise untouched, param bookkeeping untouched, l_point = state and UID = index after a failed april_graph_cholesky; the consumers
of the retained factor refuse and write nothing; and the next call on the repaired graph gives the bits of a fresh graph and param.

Measured (one MI355X), the tight cases on the chain of 90 poses, knob at the last pivot (s* = d_last):
  float64 error of d_last against the LDL' in longdouble 2.8e-12 / 9.2e-12 / 1.4e-11 (leaf_nodes 16 / 4 / 40) -> delta 1e-8 / 1e-8 / 1e-7;
  no false alarm, deviation of dx from the refined reference (max |dx| 4.3e8): LAPACK float64 6.47e5, GPU 1.41e5 (default), 6.73e5
  (small_lds_kb=0); leaf_nodes=4: 1.18e5 / 9.44e5; leaf_nodes=40 (delta 1e-7): 2.72e3 / 2.57e3.
With the in-block pivot check of chain_block removed (scratch build) the root_last@two_components and root_last@chain cases fail under every
option set but small_lds_kb=0; with the one of diag_chain32 removed the root_last cases of the random graph fail under every option set and
those of the other graphs under small_lds_kb=0; nothing faults."""
import ctypes as C

import numpy as np
import pytest

from tests.support import pivot_placement as pp
from tests.support.marginal_cases import factor_pairs
from tests.support.sigma_compare import SIG_RTOL, check_any, check_blocks, random_pairs, row_scale

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
ERR_NOT_SPD = -2
SENTINEL = -7.25

# every option set that changes the form of the factorisation ("nF-1": one front less than the graph has, as tests/test_gpu_persist_up.py
# lowers persist_max_fronts so that level 0 joins the multi-level launch)
OPTION_SETS = [dict(), dict(small_lds_kb=0), dict(small_lds_kb=48), dict(panel_mode=0, small_lds_kb=64), dict(small_threads=256),
               dict(small_threads=512), dict(tp_fronts=1, tp_lds_kb=8), dict(persist=0),
               dict(persist_up=1, persist_max_fronts="nF-1"), dict(persist_up=2, persist_max_fronts="nF-1"),
               dict(persist_up=3, persist_max_fronts="nF-1"), dict(schur_first=1), dict(leaf_nodes=4), dict(leaf_nodes=40),
               dict(use_graph=0), dict(pool_poison=1)]
# the classes of the table (first graph that offers each) + the decisive position of the graphs with several roots / a tiny root
POSITIONS = pp.CLASSES + ["root_last@two_components", "root_last@chain"]


def _ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def _lam(lib):
    p = lib.new_param(); v = float(p.c.tikhanov); p.destroy()
    return v


def _case(lib, position, leaf_nodes, **kw):
    lam = _lam(lib)
    if "@" in position:
        k, name = position.split("@")
        pl = pp.placement(lib, name, leaf_nodes, lam)
        t, c = pl.classes()[k]
    else:
        tab, missing = pp.class_table(lib, leaf_nodes, lam)
        assert not missing, missing
        pl, t, c = tab[position]
    return pl, pl.case(t, c, **kw)


def _resolve(opts, pl):
    return {k: (len(pl.ns) - 1 if v == "nF-1" else v) for k, v in opts.items()}


def _fresh(lib, arr):
    g = lib.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
    return g, p


def _set_knob(g, comp, value):
    """edit the knob (the last factor) in place: W[comp, comp] = value"""
    g.factor(g.n_factors - 1).u.W.contents.data[4 * comp] = value


def _fill_deltas(g, v):
    for i in range(g.n_nodes):
        d = g.node(i).delta_X
        d[0] = d[1] = d[2] = v


def _book(p):
    c = p.c
    return (C.cast(c.ordering, C.c_void_p).value, int(c.nreordering), int(c.factor_num))


def _snap(g):
    return g.states(), g.deltas(), g.l_points()


def _same_bits(a, b, what):
    for k, name in enumerate(("states", "deltas", "l_points")):
        assert a[k].tobytes() == b[k].tobytes(), (what, name, float(np.nanmax(np.abs(a[k] - b[k]))))


def _assert_reported(lib, p, what):
    s = p.stats()
    assert s["not_spd"] == 1, (what, s)
    assert s["error_code"] == ERR_NOT_SPD, (what, s)                   # include/aprilsam_amd.h: "-2 a pivot was not positive ... in stats.error_code
    code, msg = lib.last_error()                                        # and in aprilsam_amd_last_error"
    assert code == ERR_NOT_SPD and "not positive" in msg, (what, code, msg)


# ---- 2. detection -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leaf_nodes", pp.PLANS)
def test_the_library_eliminates_in_the_order_the_placement_assumes(lib, leaf_nodes):
    """param->ordering after a healthy call on the graph with a harmless knob = the permutation the placement model was made with"""
    for name in pp.GRAPHS:
        pl = pp.placement(lib, name, leaf_nodes, _lam(lib))
        cs = pl.case(*pl.classes()["root_last"], s_of=lambda p, d: 0.0)
        with lib.options(leaf_nodes=leaf_nodes):
            g, p = _fresh(lib, cs["arr"])
            g.cholesky(p)
            assert p.stats()["not_spd"] == 0 and p.stats()["n_fronts"] == len(pl.ns)
            assert [p.c.ordering[i] for i in range(g.n_nodes)] == pl.P.perm.tolist(), name
            p.destroy(); g.destroy()


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_ids)
@pytest.mark.parametrize("position", POSITIONS)
def test_first_non_positive_pivot_is_reported_wherever_it_sits(lib, position, opts):
    """delta = 0.25: pivot p = -0.25 d_p, every earlier pivot positive; one april_graph_cholesky on a fresh graph and param"""
    pl, cs = _case(lib, position, opts.get("leaf_nodes", 16))
    st0 = np.asarray(cs["arr"][0], float)
    lib.clear_error()
    with lib.options(**_resolve(opts, pl)):
        g, p = _fresh(lib, cs["arr"])
        _fill_deltas(g, SENTINEL)
        book = _book(p)
        g.cholesky(p)
        what = (position, opts, cs["graph"], cs["front"], cs["col"])
        _assert_reported(lib, p, what)
        st, dl, lp = _snap(g)
        assert st.tobytes() == st0.tobytes(), what
        assert np.all(dl == SENTINEL), what
        assert _book(p) == book, what
        # pinned as the code has it and as the header now says: the reference re-linearises and numbers every node before it factorises
        assert lp.tobytes() == st0.tobytes() and [g.node(i).UID for i in range(g.n_nodes)] == list(range(g.n_nodes)), what
        assert g._factorised_nodes(p) == -1
        p.destroy(); g.destroy()


def test_exact_zero_pivot_of_an_isolated_node_without_tikhonov(lib):
    st = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [5.0, 5.0, 1.0]])
    arr = (st, np.array([0, 0, 1], np.int32), np.array([-1, 1, 2], np.int32), np.array([[0, 0, 0], [1, 0.1, 0], [1, 0, 0.1]]),
           np.vstack([np.asarray([1e4, 0, 0, 0, 1e4, 0, 0, 0, 1e3]), np.tile(np.diag([10.0, 10, 10]).reshape(9), (2, 1))]))
    for opts in (dict(), dict(small_lds_kb=0)):
        lib.clear_error()
        with lib.options(**opts):
            g, p = _fresh(lib, arr)
            p.c.tikhanov = 0.0
            g.cholesky(p)
            _assert_reported(lib, p, opts)
            assert g.states().tobytes() == st.tobytes()
            p.c.tikhanov = 1e-4                      # the same param with the term back: solved
            g.cholesky(p)
            assert p.stats()["not_spd"] == 0 and p.stats()["error_code"] == 0
            assert g.states()[3].tolist() == st[3].tolist() and not np.array_equal(g.states()[:3], st[:3])
            p.destroy(); g.destroy()


# ---- the tight cases: the last pivot of the last front, s = (1 +- delta) s* -------------------------------------------------------

_TIGHT = {}


def _tight(lib, leaf_nodes):
    """chain of 90 poses (270 scalars: the graph the longer reference of tests/test_pivot_placement.py runs on).  eps = the relative
    difference of the LAST pivot between LDL' in float64 and in longdouble; delta = the smallest power of ten >= 1000 eps; s* = the
    longdouble's last pivot (for the last position s* = d_p)"""
    if leaf_nodes not in _TIGHT:
        pl = pp.placement(lib, "chain", leaf_nodes, _lam(lib))
        d64 = pp.ldl_pivots(pl.A0, np.float64); dl = pp.ldl_pivots(pl.A0, np.longdouble)
        eps = float(abs(d64[-1] - dl[-1]) / dl[-1])
        eps = max(eps, float(np.finfo(float).eps))
        delta = 10.0 ** np.ceil(np.log10(1000 * eps))
        _TIGHT[leaf_nodes] = (pl, float(dl[-1]), eps, delta)
        print(f"[tight] leaf_nodes {leaf_nodes}: float64 error of the last pivot {eps:.2e} -> delta {delta:.0e}")
    return _TIGHT[leaf_nodes]


TIGHT_OPTS = [dict(), dict(small_lds_kb=0), dict(leaf_nodes=4), dict(leaf_nodes=40), dict(use_graph=0)]


@pytest.mark.parametrize("opts", TIGHT_OPTS, ids=_ids)
def test_root_last_pivot_tight_is_reported(lib, opts):
    pl, sstar, eps, delta = _tight(lib, opts.get("leaf_nodes", 16))
    t, c = pl.classes()["root_last"]
    cs = pl.case(t, c, s_of=lambda p, d: (1 + delta) * sstar)
    assert np.nanmin(pp.ldl_pivots(pl.matrix(cs["p"], cs["s"]), np.longdouble)) < 0
    lib.clear_error()
    with lib.options(**opts):
        g, p = _fresh(lib, cs["arr"])
        g.cholesky(p)
        _assert_reported(lib, p, (opts, delta))
        assert g.states().tobytes() == np.asarray(cs["arr"][0], float).tobytes()
        p.destroy(); g.destroy()


@pytest.mark.parametrize("opts", TIGHT_OPTS, ids=_ids)
def test_no_false_alarm_just_inside_positive_definite(lib, opts):
    """s = (1 - delta) s*: solved, not reported, dx within 32 x the deviation of a plain float64 LAPACK solve (dpotrf / dpotrs in the
    plan's order) from the reference (that solve refined with longdouble residuals until it stops changing), floored at 1e-9.  32: the multifrontal order is not LAPACK's and the error
    constants grow with the front size.  Measured (module docstring): LAPACK 6.47e5 against GPU 1.41e5 / 6.73e5 at
    delta 1e-8.  The plain solve's own deviation is one draw of a spread quantity (dgetrf in the same order: 3.3e3, under which the GPU
    would read 1.3 x and 6.4 x over the bound): dpotrf is the routine for this system and the factorisation the device computes."""
    pl, sstar, eps, delta = _tight(lib, opts.get("leaf_nodes", 16))
    t, c = pl.classes()["root_last"]
    cs = pl.case(t, c, s_of=lambda p, d: (1 - delta) * sstar)
    A = pl.matrix(cs["p"], cs["s"])
    assert np.nanmin(pp.ldl_pivots(A, np.longdouble)) > 0
    xr, x0 = pp.refined_solve(A, pl.b)
    ref = np.empty(pl.n); ref[pl.idx] = np.asarray(xr, float)          # elimination order -> node order
    dev_lapack = float(np.max(np.abs(x0.astype(np.longdouble) - xr)))
    with lib.options(**opts):
        g, p = _fresh(lib, cs["arr"])
        g.cholesky(p)
        s = p.stats()
        dx = g.deltas().reshape(-1)
        p.destroy(); g.destroy()
    dev_gpu = float(np.max(np.abs(dx - ref)))
    print(f"[no false alarm] {_ids(opts)}: delta {delta:.0e} (pivot error {eps:.2e}) max|dx| {np.max(np.abs(ref)):.3e} "
          f"deviation: LAPACK float64 {dev_lapack:.3e}, GPU {dev_gpu:.3e}, allowed {max(32 * dev_lapack, 1e-9):.3e}")
    assert s["not_spd"] == 0 and s["error_code"] == 0, s
    assert np.isfinite(dx).all()
    assert dev_gpu <= max(32 * dev_lapack, 1e-9), (dev_gpu, dev_lapack)


# ---- 3. recovery ----------------------------------------------------------------------------------------------------------------

RECOVERY_POSITIONS = ["root_last", "root_last@two_components", "blk_first", "big_ob1_p3_m0"]


def _good_run(lib, arr, calls):
    """fresh graph and param on the repaired data (knob at 0), `calls` batch steps"""
    g, p = _fresh(lib, arr)
    for _ in range(calls):
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
    out = _snap(g), _book(p)[1:]
    p.destroy(); g.destroy()
    return out


@pytest.mark.parametrize("opts", [dict(), dict(use_graph=0), dict(small_lds_kb=0), dict(speculate_factors=0)], ids=_ids)
@pytest.mark.parametrize("position", RECOVERY_POSITIONS)
def test_api_calls_recover_after_a_failed_step(lib, position, opts):
    """good, good, bad (knob edited in place), good (knob edited back): the failed call changes nothing, so the last call must give the bits
    of the third call of a fresh graph and param that never saw the bad W.  From the second call on the default options launch on the
    packed factor copies while the factor objects are re-read (speculate_factors): the edit voids that run (stats.reserved1 = 1)."""
    pl, cs = _case(lib, position, 16)
    st, fa, fb, z, W = cs["arr"]
    W0 = W.copy(); W0[-1] = 0
    with lib.options(**opts):
        ref, ref_book = _good_run(lib, (st, fa, fb, z, W0), 3)
        g, p = _fresh(lib, (st, fa, fb, z, W0))
        g.cholesky(p); g.cholesky(p)
        before, book = _snap(g), _book(p)
        _set_knob(g, cs["comp"], -cs["s"])
        lib.clear_error()
        g.cholesky(p)
        _assert_reported(lib, p, (position, opts))
        if not opts:
            assert p.stats()["reserved1"] == 1            # the speculative launch was taken, and voided by the edit
        after = _snap(g)
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
        assert after[2].tobytes() == before[0].tobytes()          # l_point = the state the call came in with
        assert _book(p) == book
        _set_knob(g, cs["comp"], 0.0)
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0 and p.stats()["error_code"] == 0
        _same_bits(_snap(g), ref, (position, opts))
        assert _book(p)[1:] == ref_book
        p.destroy(); g.destroy()


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "no_sync"])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("position", ["root_last@two_components", "root_last", "leaf_c0"])
def test_resident_loop_reports_and_leaves_the_graph_alone(lib, position, steps, sync):
    """a good batch call (the param holds a factor), then begin / steps / sync on the bad system: sync returns -2, end returns -2 (also when
    no sync came before it: it reads the device's failure record itself) and the node
    objects of EVERY component keep what they held -- the failed step moves the device states of the healthy component of the
    two-component graph (the state update rides on the back substitution and does not look at the failure record).  The consumers refuse,
    and a batch call on the repaired graph gives the fresh bits."""
    d = lib.dll
    pl, cs = _case(lib, position, 16)
    st, fa, fb, z, W = cs["arr"]
    W0 = W.copy(); W0[-1] = 0
    ref, _ = _good_run(lib, (st, fa, fb, z, W0), 2)
    g, p = _fresh(lib, (st, fa, fb, z, W0))
    g.cholesky(p)
    before, book = _snap(g), _book(p)
    uid = [g.node(i).UID for i in range(g.n_nodes)]
    _set_knob(g, cs["comp"], -cs["s"])
    lib.clear_error()
    assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, steps, 0) == 0
    if sync:
        assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == ERR_NOT_SPD
    rc_end = d.aprilsam_amd_resident_end(g.ptr, p.ptr)
    _same_bits(_snap(g), before, (position, "after resident_end"))
    assert rc_end == ERR_NOT_SPD
    _assert_reported(lib, p, (position, steps))
    assert _book(p) == book and [g.node(i).UID for i in range(g.n_nodes)] == uid
    assert g._factorised_nodes(p) == -1
    out = np.full((g.n_nodes, 3, 3), SENTINEL)
    assert d.aprilsam_amd_marginals(g.ptr, p.ptr, 0, None, out.ctypes.data_as(_dp)) == -1 and np.all(out == SENTINEL)
    g.cholesky_inc(p)                                    # no factorisation at hand: returns silently (aprilsam.c:382-383)
    _same_bits(_snap(g), before, (position, "after cholesky_inc"))
    _set_knob(g, cs["comp"], 0.0)
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0 and p.stats()["error_code"] == 0
    _same_bits(_snap(g), ref, (position, "repaired"))
    p.destroy(); g.destroy()


def _refuses_everything(lib, g, p, what):
    """no factorisation: the query says -1, every consumer returns -1 and writes nothing, the incremental calls return silently"""
    assert g._factorised_nodes(p) == -1, what
    for name, (rc, outs) in _consumer_calls(lib, g, p, g.n_nodes).items():
        assert rc == -1, (what, name, rc)
        for o in outs:
            assert np.all(o == (SENTINEL if o.dtype != np.int32 else -77)), (what, name)
    before = _snap(g)
    g.cholesky_inc(p)
    g.cholesky_inc_solver(p)
    _same_bits(_snap(g), before, (what, "incremental calls without a factorisation"))


def test_resident_loop_without_a_step_after_a_failed_call(lib):
    """begin / end with no step in between, on a param whose last call failed.  The device's failure record is that call's, not the loop's, so
    end returns 0 -- and the loop factorised nothing, so it records no factorisation either: the front pool is still the failed call's,
    half written.  The param stays without one (consumers refuse, the incremental calls return silently) until a batch call succeeded, which
    then gives the bits of a fresh graph and param.  The same loop after a GOOD call leaves that call's factorisation in place."""
    pl, cs = _case(lib, "root_last@chain", 16)
    st, fa, fb, z, W = cs["arr"]
    W0 = W.copy(); W0[-1] = 0
    ref, _ = _good_run(lib, (st, fa, fb, z, W0), 1)
    g, p = _fresh(lib, cs["arr"])
    g.cholesky(p)
    assert p.stats()["not_spd"] == 1
    _set_knob(g, cs["comp"], 0.0)
    before, book = _snap(g), _book(p)
    assert lib.dll.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    assert lib.dll.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    _same_bits(_snap(g), before, "begin / end after a failed call")
    assert _book(p) == book and p.stats()["not_spd"] == 0 and p.stats()["error_code"] == 0
    _refuses_everything(lib, g, p, "begin / end after a failed call")
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0 and g._factorised_nodes(p) == g.n_nodes
    _same_bits(_snap(g), ref, "batch call after the empty loop")
    # after a good call the empty loop keeps the factorisation: the marginals before and after it are the same bits
    m0 = g.marginals(p)
    assert lib.dll.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
    assert lib.dll.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0
    assert g._factorised_nodes(p) == g.n_nodes and g.marginals(p).tobytes() == m0.tobytes()
    p.destroy(); g.destroy()


@pytest.mark.parametrize("position", ["root_last", "root_last@two_components"])
def test_resident_loop_recovers_after_a_failed_call(lib, position):
    """failed batch call, W repaired, then a whole resident loop (begin / 2 steps / sync / end): the bits of the same loop on a fresh graph and
    param, stats.not_spd = 0 and stats.error_code = 0 again, and the loop's factorisation answers (marginals against the dense inverse)"""
    from tests.test_gpu_consumer_paths import _dense_at
    d = lib.dll
    pl, cs = _case(lib, position, 16)
    st, fa, fb, z, W = cs["arr"]
    W0 = W.copy(); W0[-1] = 0

    def loop(g, p):
        assert d.aprilsam_amd_resident_begin(g.ptr, p.ptr) == 0
        assert d.aprilsam_amd_resident_steps(g.ptr, p.ptr, 2, 0) == 0
        assert d.aprilsam_amd_resident_sync(g.ptr, p.ptr) == 0
        assert d.aprilsam_amd_resident_end(g.ptr, p.ptr) == 0

    gr, pr = _fresh(lib, (st, fa, fb, z, W0))
    loop(gr, pr)
    ref = _snap(gr)
    pr.destroy(); gr.destroy()
    g, p = _fresh(lib, cs["arr"])
    lib.clear_error()
    g.cholesky(p)
    _assert_reported(lib, p, position)
    _set_knob(g, cs["comp"], 0.0)
    loop(g, p)
    s = p.stats()
    assert s["not_spd"] == 0 and s["error_code"] == 0, s
    _same_bits(_snap(g), ref, (position, "resident loop after a failed call"))
    assert g._factorised_nodes(p) == g.n_nodes
    dense = _dense_at(g.l_points(), (st, fa, fb, z, W0), _lam(lib))
    assert check_blocks(dense, fa, fb, g.marginals(p), g.marginals_joint(p, *factor_pairs(fa, fb))) < SIG_RTOL
    p.destroy(); g.destroy()


def test_batch_resident_wrapper_reports(lib):
    pl, cs = _case(lib, "root_last@two_components", 16)
    g, p = _fresh(lib, cs["arr"])
    st0 = _snap(g)
    chi2 = np.zeros(3); ms = np.zeros(2)
    assert lib.dll.aprilsam_amd_batch_resident(g.ptr, p.ptr, 2, chi2.ctypes.data_as(_dp), ms.ctypes.data_as(_dp)) == ERR_NOT_SPD
    _same_bits(_snap(g), st0, "batch_resident")
    assert g._factorised_nodes(p) == -1 and p.stats()["not_spd"] == 1
    p.destroy(); g.destroy()


@pytest.mark.parametrize("opts", [dict(), dict(inc_one=0, inc_tail=0)], ids=_ids)
@pytest.mark.parametrize("position", ["root_last", "leaf_c0", "middle_level"])
def test_incremental_call_after_a_failed_batch_step_has_no_factor_to_extend(lib, position, opts):
    """good batch, bad batch, repair, april_graph_cholesky_inc with one new factor.  The failed batch step stopped with fronts half written:
    an incremental step that regenerated only the new factor's root path would solve with the rest of that pool.  The failed call drops the
    factorisation (as the failed incremental call always did for tail_ok / upd_ok), so the incremental call returns silently, as the header
    says for any failure, and the batch call that follows gives the bits of a fresh graph and param."""
    pl, cs = _case(lib, position, 16)
    st, fa, fb, z, W = cs["arr"]
    W0 = W.copy(); W0[-1] = 0
    N = len(st)
    a, b = 3, N - 5
    newz = np.array([st[b, 0] - st[a, 0], st[b, 1] - st[a, 1], 0.0]); newW = np.diag([20.0, 20.0, 50.0])
    with lib.options(deterministic=1, **opts):
        # reference: fresh graph and param, good batch, then the new factor and a batch call
        gr, pr = _fresh(lib, (st, fa, fb, z, W0))
        gr.cholesky(pr)
        gr.add_factor_xyt(a, b, newz, newW)
        gr.cholesky(pr)
        ref = _snap(gr)
        pr.destroy(); gr.destroy()

        g, p = _fresh(lib, (st, fa, fb, z, W0))
        g.cholesky(p)
        before = _snap(g)
        _set_knob(g, cs["comp"], -cs["s"])
        lib.clear_error()
        g.cholesky(p)
        _assert_reported(lib, p, (position, opts))
        _set_knob(g, cs["comp"], 0.0)
        g.add_factor_xyt(a, b, newz, newW)
        g.cholesky_inc(p)
        after = _snap(g)
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes(), (position, opts)
        assert np.isfinite(after[0]).all()
        g.cholesky_inc_solver(p)
        assert g.states().tobytes() == before[0].tobytes()
        g.cholesky(p)
        assert p.stats()["not_spd"] == 0
        _same_bits(_snap(g), ref, (position, opts))
        p.destroy(); g.destroy()


@pytest.mark.parametrize("opts", [dict(), dict(inc_one=0, inc_tail=0)], ids=_ids)
def test_incremental_step_with_an_indefinite_closure(lib, oracle, opts):
    """good batch, an incremental step whose new closure carries an indefinite W (reported, everything untouched), W repaired; the param has
    no factorisation until the next batch step (the incremental call returns silently), after which incremental steps are exact again --
    every successful step checked against its exact linear system by tests/support/inc_exact.py."""
    from tests.support.inc_exact import IncExact
    arr = pp.graph("chain")
    st = arr[0]; N = len(st)
    with lib.options(deterministic=1, **opts):
        chk = IncExact(lib, oracle)
        g = chk.new_graph(); g.build_from_arrays(*arr); p = lib.new_param()
        g.cholesky(p)
        before = _snap(g.g)
        a, b = 10, 70
        zz = np.array([st[b, 0] - st[a, 0], st[b, 1] - st[a, 1], 0.0])
        g.add_factor_xyt(a, b, zz, np.diag([-1e6, 20.0, 50.0]))
        lib.clear_error()
        g.g.cholesky_inc(p)                              # (raw: the checker's model has no failed steps)
        _assert_reported(lib, p, opts)
        _same_bits(_snap(g.g), before, "failed incremental step")
        Wd = g.g.factor(g.g.n_factors - 1).u.W.contents.data
        Wd[0] = 20.0
        g.g.cholesky_inc(p)                              # nothing to extend: silent
        _same_bits(_snap(g.g), before, "incremental call without a factorisation")
        g.cholesky(p)                                    # batch step, residual checked
        g.add_factor_xyt(20, 60, np.array([st[60, 0] - st[20, 0], st[60, 1] - st[20, 1], 0.0]), np.diag([20.0, 20.0, 50.0]))
        g.cholesky_inc(p)                                # exact incremental step
        assert p.stats()["not_spd"] == 0 and chk.report["failures"] == 0 and chk.report["inc"] + chk.report["fallback"] == 1, chk.summary()
        p.destroy(); g.destroy()


# ---- Levenberg-Marquardt: the step is rejected, not the call ---------------------------------------------------------------------------

@pytest.mark.parametrize("opts", [dict(), dict(small_lds_kb=0), dict(use_graph=0)], ids=_ids)
@pytest.mark.parametrize("position,delta", pp.LM_CASES)
def test_lm_rejects_what_the_model_rejects(lib, position, delta, opts):
    """aprilsam_amd_optimize_lm on the chain with the indefinite prior against tests/support/lm_model.py with its rejection branch: the count
    rejected_not_spd and the accept / reject sequence exactly, lambda per iteration at 1e-6, F of the accepted steps, the final F and the final
    states at 1e-9 (the tolerances of tests/test_gpu_lm.py).  No model decision lies within LM_MARGIN of a zero pivot."""
    from tests.support import lm_model as M
    pl, cs = _case(lib, position + "@chain", 16, delta=delta)
    st, fa, fb, z, W = cs["arr"]
    ref = M.optimize(st, (fa, fb, z, W), max_iters=pp.LM_ITERS, spd_check=pp.ldl_pivots)
    assert ref["margins"].min() > pp.LM_MARGIN and ref["rejected_not_spd"] >= 4
    with lib.options(**opts):
        g, p = _fresh(lib, cs["arr"])
        r = g.optimize_lm(p, trace=True, max_iters=pp.LM_ITERS)
        x = g.states()
        p.destroy(); g.destroy()
    t, rt = r["trace"], ref["trace"]
    print(f"[lm] {position} {_ids(opts)}: not_spd {r['rejected_not_spd']} / {ref['rejected_not_spd']} accepted {r['accepted']} / {ref['accepted']} "
          f"lambda {np.max(np.abs(t[:, 2] / rt[:, 2] - 1)):.2e} F_final {r['F_final']:.9e} / {ref['F_final']:.9e}")
    assert r["rejected_not_spd"] == ref["rejected_not_spd"] and r["iterations"] == ref["iterations"] and r["status"] == ref["status"]
    assert np.array_equal(t[:, 3], rt[:, 3]), (t[:, 3], rt[:, 3])
    assert np.all(np.abs(t[:, 2] - rt[:, 2]) <= 1e-6 * np.abs(rt[:, 2]))
    acc = rt[:, 3] == 1
    assert np.all(np.abs(t[acc, 0] - rt[acc, 0]) <= 1e-9 * np.abs(rt[acc, 0]))
    assert abs(r["F_final"] - ref["F_final"]) <= 1e-9 * abs(ref["F_final"]) and r["accepted"] == ref["accepted"]
    e = x - ref["x"]; e[:, 2] = M.mod2pi(e[:, 2])
    assert np.abs(e).max() < 1e-9, np.abs(e).max()


def test_gnc_over_a_graph_with_the_indefinite_prior(lib):
    """aprilsam_amd_optimize_gnc with xyt candidates elsewhere on the chain: what its header documents holds although stages reject steps
    for a non-positive pivot -- the call returns 0 with status 1 or 2, two runs give identical bits, state = l_point, the retained factor
    is dropped, no factor object is modified, and (the knob edited back) a following april_graph_cholesky gives the bits it gives on a
    fresh copy of the graph at the same states."""
    pl, cs = _case(lib, "root_last@chain", 16, delta=4.0)     # (LM_CASES[0]: four rejections for the pivot at lambda0, then accepted steps)
    st, fa, fb, z, W = cs["arr"]
    cand = np.arange(20, 40, dtype=np.int32)                 # odometry factors away from the knob's pose
    assert cs["node"] not in set(fa[cand]) | set(fb[cand])
    runs = []
    for _ in range(2):
        g, p = _fresh(lib, cs["arr"])
        r = g.optimize_gnc(p, cand, trace=True, max_stages=4, max_iters=10)
        runs.append((r, _snap(g), g, p))
    (r, snap, g, p), (r2, snap2, g2, p2) = runs
    assert r["status"] in (1, 2) and 1 <= r["stages"] <= 4 and r["iterations"] >= r["accepted"] >= 1
    assert {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in r.items()} == {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in r2.items()}
    _same_bits(snap, snap2, "two GNC runs")
    assert np.isfinite(snap[0]).all() and snap[0].tobytes() == snap[2].tobytes()
    assert g._factorised_nodes(p) == -1
    arr_after = g.arrays()
    assert arr_after[4].tobytes() == np.ascontiguousarray(W, float).tobytes() and arr_after[3].tobytes() == np.ascontiguousarray(z, float).tobytes()
    _set_knob(g, cs["comp"], 0.0)
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0
    W0 = W.copy(); W0[-1] = 0
    gf, pf = _fresh(lib, (snap[0], fa, fb, z, W0))
    gf.cholesky(pf)
    _same_bits(_snap(g), _snap(gf), "batch step after GNC against a fresh copy")
    for a, b in ((g, p), (g2, p2), (gf, pf)):
        b.destroy(); a.destroy()


# ---- consumers of the retained factor after a failed step ---------------------------------------------------------------------------

_POLAR_KINDS = [3, 1, 2, 3]                    # range-bearing, range, bearing, range-bearing (tests/support/polar_model.py)
_POLAR_Z, _POLAR_W = [1.0, 0.1], [25.0, 3.0, 3.0, 100.0]
_GATE_Z, _GATE_W = [1.0, 0.0, 0.0], np.diag([10.0, 10.0, 40.0])


def _polar_cands():
    """the polar candidates of _consumer_calls as the model takes them: (kind, z [m], W [m, m]); a 1-row kind uses z[0] and W[0]"""
    W2 = np.array(_POLAR_W).reshape(2, 2)
    return [(k, np.array(_POLAR_Z), W2) if k == 3 else (k, np.array(_POLAR_Z[:1]), W2[:1, :1]) for k in _POLAR_KINDS]


def _consumer_calls(lib, g, p, N):
    """every consumer through the C entry points with sentinel-filled outputs -> {name: (rc, outputs)}"""
    d = lib.dll
    ia = lambda v: np.ascontiguousarray(v, np.int32)
    I = lambda v: v.ctypes.data_as(_ip)
    D = lambda v: v.ctypes.data_as(_dp)
    full = lambda *shape: np.full(shape, SENTINEL)
    res = {}
    a, b = ia([0, 5, N - 1, 7]), ia([N - 1, 6, 0, 8])
    n = len(a)
    o = full(N, 3, 3); res["marginals"] = (d.aprilsam_amd_marginals(g.ptr, p.ptr, 0, None, D(o)), [o])
    o = full(n, 6, 6); res["joint_any"] = (d.aprilsam_amd_marginals_joint_any(g.ptr, p.ptr, n, I(a), I(b), D(o)), [o])
    z = np.tile(_GATE_Z, (n, 1)); Wg = np.tile(_GATE_W.reshape(9), (n, 1))
    d2, S = full(n), full(n, 3, 3)
    res["gate_xyt"] = (d.aprilsam_amd_gate_xyt(g.ptr, p.ptr, n, I(a), I(b), D(z), D(Wg), D(d2), D(S)), [d2, S])
    kind = ia(_POLAR_KINDS); zp = np.tile(_POLAR_Z, (n, 1)); Wp = np.tile(_POLAR_W, (n, 1))
    a2, b2 = ia([0, 5, N - 1, 7]), ia([N - 1, 6, 0, 8])
    d2, S = full(n), full(n, 2, 2)
    res["gate_polar"] = (d.aprilsam_amd_gate_polar(g.ptr, p.ptr, n, I(a2), I(b2), I(kind), D(zp), D(Wp), D(d2), D(S)), [d2, S])
    lm = ia([1, 2, 3]); dm, best, db, ds = full(n, 3), np.full(n, -77, np.int32), full(n), full(n)
    res["associate_polar"] = (d.aprilsam_amd_associate_polar(g.ptr, p.ptr, 0, n, I(kind), D(zp), D(Wp), 3, I(lm), 9.0, 1.0, D(dm), I(best), D(db), D(ds)),
                              [dm, best, db, ds])
    B = np.ones((1, 3 * N)); X = full(1, 3 * N)
    res["solve"] = (d.aprilsam_amd_solve(g.ptr, p.ptr, 0, 1, D(B), D(X)), [X])
    nodes = ia([1, N - 2])
    o = full(2, 3, 3); res["cross"] = (d.aprilsam_amd_marginals_cross(g.ptr, p.ptr, 0, 2, I(nodes), D(o)), [o])
    o = full(2, 3, 3); res["relative"] = (d.aprilsam_amd_relative_covariances(g.ptr, p.ptr, 0, 2, I(nodes), D(o)), [o])
    return res


@pytest.mark.parametrize("position", ["root_last", "root_last@two_components"])
def test_consumers_refuse_after_a_failed_step_and_answer_after_the_repair(lib, position):
    from tests.test_gpu_consumer_paths import _dense_at
    pl, cs = _case(lib, position, 16)
    st, fa, fb, z, W = cs["arr"]
    W0 = W.copy(); W0[-1] = 0
    N = len(st)
    g, p = _fresh(lib, (st, fa, fb, z, W0))
    g.cholesky(p)
    assert g._factorised_nodes(p) == N
    good = _consumer_calls(lib, g, p, N)
    assert all(rc >= 0 for rc, _ in good.values()), {k: rc for k, (rc, _) in good.items()}
    _set_knob(g, cs["comp"], -cs["s"])
    g.cholesky(p)
    assert p.stats()["not_spd"] == 1
    assert g._factorised_nodes(p) == -1
    for name, (rc, outs) in _consumer_calls(lib, g, p, N).items():
        assert rc == -1, (name, rc)                                                        # "no retained factor"
        for o in outs:
            assert np.all(o == (SENTINEL if o.dtype != np.int32 else -77)), name            # nothing written
    _set_knob(g, cs["comp"], 0.0)
    g.cholesky(p)
    assert p.stats()["not_spd"] == 0 and g._factorised_nodes(p) == N
    lp = g.l_points()
    ref = _dense_at(lp, (st, fa, fb, z, W0), _lam(lib))
    Sig = ref[0]
    a, b = random_pairs(N, 1)
    assert check_blocks(ref, fa, fb, g.marginals(p), g.marginals_joint(p, *factor_pairs(fa, fb))) < SIG_RTOL
    assert check_any(ref, a, b, g.marginals_joint_any(p, a, b)) < SIG_RTOL
    after = _consumer_calls(lib, g, p, N)
    assert all(rc >= 0 for rc, _ in after.values())
    X = after["solve"][1][0].reshape(-1)
    Xr = Sig @ np.ones(3 * N)
    assert np.max(np.abs(X - Xr)) <= 1e-9 * np.max(np.abs(Xr))
    cross = after["cross"][1][0]
    for k, n in enumerate([1, N - 2]):
        blk = Sig[3 * n:3 * n + 3, 0:3]
        assert np.max(np.abs(cross[k] - blk)) <= 1e-9 * max(row_scale(Sig)[n], row_scale(Sig)[0])
    # the gates and the relative covariances against their numpy models on the blocks of the DENSE inverse of the repaired system, at the
    # tolerances of the tests that own them (tests/test_gpu_gating.py, test_gpu_polar_gate.py, test_gpu_treesolve.py: GATE_RTOL = 1e-9; the
    # xyt gate on the dense blocks 1e-7 of every d2, on the library's own joint blocks -- held to the dense inverse above -- 1e-9): the states
    # and l_points differ from those of the factorisation before the failed call, so a Sigma pool or a path-solve cache that outlived it fails
    from tests.support import gate_model, polar_gate_model as pg
    from tests.support.sigma_compare import ref_joint
    from tests.support.treesolve_model import relative_covariances
    GATE_RTOL = 1e-9
    x = g.states()
    assert not np.array_equal(x, st) and not np.array_equal(lp, st)
    pa_, pb_ = np.array([0, 5, N - 1, 7], np.int32), np.array([N - 1, 6, 0, 8], np.int32)          # (the pairs of _consumer_calls)
    n = len(pa_)
    gz, gW = np.tile(_GATE_Z, (n, 1)), np.tile(_GATE_W.reshape(9), (n, 1))
    d2, S = after["gate_xyt"][1]
    md2, mS = gate_model.gate(x, pa_, pb_, gz, gW, g.marginals_joint_any(p, pa_, pb_))
    assert (np.abs(d2 - md2) <= GATE_RTOL * np.abs(md2)).all() and np.abs(S - mS).max() < GATE_RTOL * np.abs(mS).max()
    md2, mS = gate_model.gate(x, pa_, pb_, gz, gW, ref_joint(Sig, pa_, pb_))
    assert (np.abs(d2 - md2) <= 1e-7 * np.abs(md2)).all() and np.abs(S - mS).max() <= 1e-7 * np.abs(mS).max()
    cands = _polar_cands()
    rc, (d2, S) = after["gate_polar"]
    ok, md2, mS = pg.gate(x, pa_, pb_, cands, pg.joint_blocks(Sig, pa_, pb_))
    mS = pg.padded(mS)
    assert rc == 0 and ok.all()
    assert (np.abs(d2 - md2) <= GATE_RTOL * np.abs(md2)).all() and np.abs(S - mS).max() < GATE_RTOL * np.abs(mS).max()
    rc, (dm, best, db, ds) = after["associate_polar"]
    lms = np.array([1, 2, 3], np.int32)
    m = pg.associate(x, 0, cands, lms, pg.joint_blocks(Sig, [0] * len(lms), lms), 9.0, 1.0)
    assert rc == m["unavailable"] == 0 and np.array_equal(best, m["best"])
    assert (np.abs(dm - m["d2"]) <= GATE_RTOL * np.abs(m["d2"])).all()
    assert (np.abs(db - m["d2_best"]) <= GATE_RTOL * np.abs(m["d2_best"])).all() and (np.abs(ds - m["d2_second"]) <= GATE_RTOL * np.abs(m["d2_second"])).all()
    R = after["relative"][1][0]
    nodes = np.array([1, N - 2])
    Sii = np.stack([Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in nodes])
    Sia = np.stack([Sig[3 * i:3 * i + 3, 0:3] for i in nodes])
    model = relative_covariances(x, 0, nodes, Sig[0:3, 0:3], Sii, Sia)
    big = np.abs(model).max(axis=(1, 2))
    assert (np.abs(R - model).max(axis=(1, 2)) / big).max() < GATE_RTOL
    p.destroy(); g.destroy()
