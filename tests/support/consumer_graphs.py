"""Graphs of tests/test_gpu_consumer_paths.py and tests/test_front_census.py beyond tests/support/marginal_cases.py.  TEST-ONLY."""
import numpy as np

from aprilsam_amd import datasets


def joined(*parts):
    """disjoint union of pose graphs (states, fa, fb, z, W): the node ids of each part shifted behind the parts before it; every
    part keeps its own prior, so the union has one root (at least) per part"""
    st, fa, fb, z, W = [], [], [], [], []
    off = 0
    for s, a, b, zz, WW in parts:
        a = np.asarray(a, np.int32); b = np.asarray(b, np.int32)
        st.append(np.asarray(s, float)); fa.append(a + off); fb.append(np.where(b >= 0, b + off, b).astype(np.int32))
        z.append(np.asarray(zz, float).reshape(-1, 3)); W.append(np.asarray(WW, float).reshape(-1, 9))
        off += len(s)
    return np.vstack(st), np.concatenate(fa).astype(np.int32), np.concatenate(fb).astype(np.int32), np.vstack(z), np.vstack(W)


def lone_pose():
    """one pose with only a prior"""
    return (np.array([[3.0, -2.0, 0.5]]), np.array([0], np.int32), np.array([-1], np.int32), np.array([[3.1, -2.1, 0.45]]),
            np.asarray(datasets.PRIOR_W, float).reshape(1, 9))


def component_of(parts):
    """component index of every node of joined(*parts)"""
    return np.concatenate([np.full(len(p[0]), k) for k, p in enumerate(parts)])


def two_components():
    parts = (datasets.random_pose_graph(400, 350, 2), datasets.random_pose_graph(80, 60, 1))
    return joined(*parts), component_of(parts)


def three_components():
    parts = (datasets.random_pose_graph(400, 350, 2), datasets.random_pose_graph(80, 60, 1), lone_pose())
    return joined(*parts), component_of(parts)
