"""The shared dense-Sigma comparison of the GPU tests (tests/support/sigma_compare.py) discriminates: on the numpy Sigma of a small
graph it passes against itself and fails for one diagonal block off by 1e-7 of its row scale, for lambda on the wrong node set and for
one transposed joint block.  No GPU: a stand-in graph returns blocks cut from a dense matrix."""
import types

import numpy as np
import pytest

from aprilsam_amd import datasets
from tests.support import sigma_compare as S
from tests.support.marginal_cases import LAM, factor_pairs
from tests.support.selinv_model import dense_system, system_blocks


class _Graph:
    """answers the calls compare_dense / compare_dense_any make, from a dense Sigma"""
    def __init__(self, arr, lam_nodes=None):
        self.arr = arr
        states, fa, fb, z, W = arr
        Aii, Aab = system_blocks(states, fa, fb, z, W, LAM, lam_nodes)
        self.Sig = np.linalg.inv(dense_system(Aii, Aab, fa, fb))
        self.edit = lambda kind, blocks: blocks

    def arrays(self):
        return self.arr

    def l_points(self):
        return self.arr[0]

    def marginals(self, p):
        return self.edit("diag", S.ref_blocks(self.Sig, len(self.arr[0]), self.arr[1], self.arr[2])[0].copy())

    def marginals_joint(self, p, a, b):
        return self.edit("joint", S.ref_joint(self.Sig, a, b).copy())

    def marginals_joint_any(self, p, a, b):
        return self.edit("any", S.ref_joint(self.Sig, a, b).copy())


PARAM = types.SimpleNamespace(c=types.SimpleNamespace(tikhanov=LAM))
ARR = datasets.random_pose_graph(80, 60, 1)


def _pairs():
    fa, fb = factor_pairs(ARR[1], ARR[2])
    a, b = S.random_pairs(len(ARR[0]), 1)
    return np.r_[a, fa].astype(np.int32), np.r_[b, fb].astype(np.int32)


def test_passes_against_itself():
    g = _Graph(ARR)
    assert S.compare_dense(g, PARAM) < 1e-13
    S.compare_dense_any(g, PARAM, *_pairs())
    n = 30                                       # lambda on the first n nodes only, on both sides
    g = _Graph(ARR, n)
    S.compare_dense(g, PARAM, n); S.compare_dense_any(g, PARAM, *_pairs(), n)


def test_fails_for_one_diagonal_block_off_by_1e_7_of_its_row_scale():
    g = _Graph(ARR)
    scale = S.row_scale(g.Sig)

    def edit(kind, blocks):
        if kind == "diag":
            blocks[37, 1, 2] += 1e-7 * scale[37]
        return blocks
    g.edit = edit
    with pytest.raises(AssertionError):
        S.compare_dense(g, PARAM)


def test_fails_for_lambda_on_the_wrong_node_set():
    n = 30
    for have, want in ((None, n), (n, None), (n, n + 1)):
        g = _Graph(ARR, have)
        with pytest.raises(AssertionError):
            S.compare_dense(g, PARAM, want)
        with pytest.raises(AssertionError):
            S.compare_dense_any(g, PARAM, *_pairs(), want)


@pytest.mark.parametrize("kind", ["joint", "any"])
def test_fails_for_one_transposed_joint_block(kind):
    g = _Graph(ARR)

    def edit(k, blocks):
        if k == kind:
            blocks[5, :3, 3:] = blocks[5, :3, 3:].T.copy()          # Sigma_ab for Sigma_ba (and the other way round)
            blocks[5, 3:, :3] = blocks[5, :3, 3:].T
        return blocks
    g.edit = edit
    a, b = _pairs()
    assert a[5] != b[5]
    with pytest.raises(AssertionError):
        S.compare_dense(g, PARAM) if kind == "joint" else S.compare_dense_any(g, PARAM, a, b)
