"""Degenerate tree shapes: a star (one separator, every other pose a child of the root front) and a chain (deep, thin elimination tree).
TEST-ONLY; used by tests/test_gpu_parity.py and tests/support/shard_designs.py."""
import numpy as np

from aprilsam_amd import datasets


def _star(n_leaves, seed):
    """hub 0 connected to every other pose: one separator (the hub), n_leaves children of the root front"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-np.pi, np.pi, n_leaves); rad = rng.uniform(1, 20, n_leaves)
    st = np.vstack([[0, 0, 0], np.column_stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-np.pi, np.pi, n_leaves)])])
    fa = np.zeros(n_leaves, np.int32); fb = np.arange(1, n_leaves + 1, dtype=np.int32)
    z = np.column_stack([st[1:, 0] + rng.normal(0, .1, n_leaves), st[1:, 1] + rng.normal(0, .1, n_leaves), st[1:, 2] + rng.normal(0, .02, n_leaves)])
    W = np.tile(np.diag([50.0, 50.0, 200.0]).reshape(9), (n_leaves, 1))
    return datasets.with_prior(st, fa, fb, z, W, first=True)


def _chain(n, seed):
    rng = np.random.default_rng(seed)
    st = np.column_stack([np.arange(n, dtype=float), rng.normal(0, .2, n), rng.normal(0, .05, n)])
    fa = np.arange(n - 1, dtype=np.int32); fb = fa + 1
    z = np.column_stack([np.ones(n - 1), np.zeros(n - 1), np.zeros(n - 1)])
    W = np.tile(np.diag([100.0, 100.0, 400.0]).reshape(9), (n - 1, 1))
    return datasets.with_prior(st, fa, fb, z, W, first=False)
