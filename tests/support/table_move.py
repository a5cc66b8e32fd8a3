"""A pose chain grown through april_graph_cholesky_inc while factors of ONE family (max-mixture or robust) are appended a few per step,
so that the family's device table runs out of room and moves in the middle of the run.  TEST INFRASTRUCTURE for
tests/test_gpu_maxmix.py and tests/test_gpu_robust.py.

The values a kernel wrote into the table (the component k_select_mixture chose, the weight k_robust_weight applied) exist only on the
device: the host holds a value only for factors it linearised itself (select_new_max / select_new_robust; -1 otherwise).  A batch step
linearises every factor on the device, so after it the host's values are stale for every factor packed so far -- a move that did not
read the device's values back first would hand the stale ones out again.

How many factors make a table move.  A device buffer grows to max(n, cap + cap / 2) when asked for n > cap elements (DBuf::need).  The
first upload is the first batch step's, with the 6 factors of EARLY.
- Asked for n + n / 2 + 64 rows (the robust table's rule): 6 + 3 + 64 = 73 rows, so the table moves when the 74th factor arrives, to
  74 + 37 + 64 = 175 rows: once in a run of 140 factors.  The same rule on the max factors' components (two per factor): 12 + 6 + 64 = 82
  components, 41 factors.
- Asked for exactly the rows needed (the max table's rule on commit 362a7eb): 6, then 9, 13, 19, 28, 42, 63, 94, 141 rows -- a move
  whenever the count passes one of them (and more in between, where the component buffers run out).
ROW_CAPS lists these capacities: a test asserts that the step which takes the count past each of them is a fast-path step.  The batch
step of REBATCH_AT comes at the 56th factor, so every move behind it finds at least 56 device-written values whose host copies are stale."""
import numpy as np

from tests.support import polar_model as pm

POSES, FIRST_BATCH, REBATCH_AT = 118, 10, 50
FAMILY_FACTORS_MIN = 100
ROW_CAPS = dict(robust=(73,), max=(9, 13, 19, 28, 41, 42, 63, 73, 94))
EARLY = [(0, 5), (2, 8), (1, 9), (3, 10), (4, 7), (0, 10)]      # family factors of the first batch step


def scene(seed):
    """poses along a gentle arc, measurements from the truth with noise; every third family factor gets a measurement that is off by
    half a metre (the null component wins / the weight is well below 1)"""
    rng = np.random.default_rng(seed)
    t = np.arange(POSES)
    truth = np.column_stack([0.5 * t, 2.0 * np.sin(0.1 * t), 0.2 * np.cos(0.1 * t)])
    start = truth + np.column_stack([rng.normal(0, 0.02, (POSES, 2)), rng.normal(0, 0.01, POSES)])

    def meas(a, b, off=0.0):
        q, _, _ = pm.rel(truth[a], truth[b])
        return np.array([q[0] + off + rng.normal(0, 0.02), q[1] + rng.normal(0, 0.02), pm.mod2pi(truth[b, 2] - truth[a, 2] + rng.normal(0, 0.01))])
    return dict(start=start, meas=meas, W=np.diag([100.0, 100.0, 400.0]))


def grow(lib, sc, add_family, query):
    """add_family(g, a, b, z, W): appends one family factor; query(g, p, idx): the device-written values of the listed factors.
    -> dict(steps, fast, spans, family, checked, values): incremental steps made, how many took the fast path and the family's factor
    count before and after each of those, family factors at the end, how many (step, factor) pairs were compared, the final values.
    Asserts that every fast-path step leaves the values of all older family factors as they were."""
    g = lib.new_graph(); p = lib.new_param(nthreshold=10 ** 6)
    fam = []                                                    # graph indices of the family's factors
    count = [0]

    def family(a, b):
        count[0] += 1
        add_family(g, a, b, sc["meas"](a, b, 0.5 if count[0] % 3 == 0 else 0.0), sc["W"])
        fam.append(g.n_factors - 1)

    steps = fast = checked = 0
    spans = []                                                  # (family factors before, after) of every fast-path step
    for n in range(POSES):
        g.add_node_xyt(sc["start"][n])
        if n == 0:
            g.add_factor_xytpos(0, sc["start"][0], sc["W"])
        else:
            g.add_factor_xyt(n - 1, n, sc["meas"](n - 1, n), sc["W"])
        if n == FIRST_BATCH:
            for a, b in EARLY:
                family(a, b)
            g.cholesky(p)
            assert np.all(query(g, p, fam) != -1)                   # the batch step linearised them on the device
            continue
        if n < FIRST_BATCH:
            continue
        family(n - 3, n)                                            # a few per step: one, and a second on every fourth step
        if n % 4 == 0:
            family(n - 7, n)
        if n == REBATCH_AT:                                         # a batch step in the middle: every value so far is now device-written
            g.cholesky(p)
            continue
        old = fam[:-2] if n % 4 == 0 else fam[:-1]
        assert len(old) >= len(EARLY)
        before = query(g, p, old)
        bt = 1e300; p.c.batch_time = bt
        g.cholesky_inc(p)
        steps += 1
        after = query(g, p, old)
        assert np.all(query(g, p, fam) != -1), n                    # the new ones were linearised by the step
        if p.c.batch_time == bt and p.stats()["inc_replanned"] == 0:      # (a re-planned step or a fall-back linearises everything again)
            fast += 1; checked += len(old); spans.append((len(old), len(fam)))
            assert before.tobytes() == after.tobytes(), (n, np.nonzero(before != after)[0])
    out = dict(steps=steps, fast=fast, spans=spans, family=len(fam), checked=checked, values=query(g, p, fam))
    p.destroy(); g.destroy()
    return out
