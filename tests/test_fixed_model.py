"""The numpy restatement of fixed nodes (tests/support/fixed_model.py) pinned on the CPU: the masked full solve
equals the reduced solve padded with zeros, on the graphs and fixed sets the GPU tests use.  No GPU."""
import numpy as np
import pytest

from tests.support import fixed_model as fm


@pytest.fixture(scope="module")
def chain():
    return fm.chain8()


@pytest.mark.parametrize("fixed", fm.FIXED_SETS, ids=str)
@pytest.mark.parametrize("lam", [1e-4, 0.0])
def test_masked_full_solve_equals_reduced_solve(chain, fixed, lam):
    A, B = fm.system(chain["start"], chain["plain"], lam=lam)
    Am, Bm = fm.mask(A, B, fixed)
    idx = fm.dofs(fixed)
    free = np.setdiff1d(np.arange(len(B)), idx)
    # the mask: fixed rows / columns / rhs zero, diagonal exactly 1, everything else the unmasked system's bits
    assert np.array_equal(Am[np.ix_(idx, idx)], np.eye(len(idx))) and not Am[np.ix_(idx, free)].any() and not Am[np.ix_(free, idx)].any()
    assert not Bm[idx].any()
    assert np.array_equal(Am[np.ix_(free, free)], A[np.ix_(free, free)]) and np.array_equal(Bm[free], B[free])
    d_full = fm.masked_solve(A, B, fixed)
    d_red = fm.reduced_solve(A, B, fixed)
    assert np.all(d_full[idx] == 0.0) and np.all(d_red[idx] == 0.0)
    scale = max(1.0, np.abs(d_red).max())
    assert np.abs(d_full - d_red).max() <= 1e-12 * scale
    # a free node next to a fixed one keeps the whole H_bb of the factor between them: the reduced system is NOT the graph without that factor
    assert np.array_equal(np.diag(Am)[free], np.diag(A)[free])


def test_relative_only_graph_is_regular_with_node_0_fixed(chain):
    fa, fb, z, W = chain["plain"]
    rel = tuple(v[fb >= 0] for v in (fa, fb, z, W))            # the prior dropped: a gauge freedom of dimension 3
    A, B = fm.system(chain["start"], rel, lam=0.0)
    ev = np.linalg.eigvalsh(A)
    assert ev[2] < 1e-8 * ev[-1] < ev[3]                       # singular as it stands ...
    Am, _ = fm.mask(A, B, (0,))
    assert np.linalg.eigvalsh(Am)[0] > 1e-6                    # ... regular and exact with node 0 fixed
    d = fm.reduced_solve(A, B, (0,))
    assert np.all(np.isfinite(d)) and np.all(d[:3] == 0.0)


def test_step_and_wrap(chain):
    x = chain["start"]
    assert np.all(fm.unchanged_by_wrap(x[:, 2]))
    A, B = fm.system(x, chain["plain"], lam=1e-4)
    d = fm.reduced_solve(A, B, (0, 7))
    x1 = fm.step(x, d)
    assert x1[0].tobytes() == x[0].tobytes() and x1[7].tobytes() == x[7].tobytes()
    assert not np.array_equal(x1[1:7], x[1:7])
    # a heading outside [-pi, pi) comes back wrapped, whoever holds it
    assert abs(fm.mod2pi(4.0) - (4.0 - 2 * np.pi)) < 1e-15 and not fm.unchanged_by_wrap(4.0)


def test_conditional_covariance(chain):
    A, _ = fm.system(chain["start"], chain["plain"], lam=1e-4)
    S = fm.conditional_covariance(A, (0, 7))
    idx = fm.dofs((0, 7))
    assert not S[idx, :].any() and not S[:, idx].any()
    Am, _ = fm.mask(A, np.zeros(len(A)), (0, 7))
    Sm = np.linalg.inv(Am)
    free = np.setdiff1d(np.arange(len(A)), idx)
    assert np.abs(Sm[np.ix_(free, free)] - S[np.ix_(free, free)]).max() <= 1e-12 * np.abs(S).max()
