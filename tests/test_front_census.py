"""Which front shapes the graphs of tests/test_gpu_consumer_paths.py put in front of the consumers of the retained factor (selected
inversion, path solves), from the library's own plan at default options: s = scalar columns a front owns (L_SS is s x s), u = scalar
rows of its update block (L_US is u x s).  The union must hold every class the kernels treat differently; a class that goes missing
gets a graph added to the GPU tests, never dropped from this list."""
import numpy as np

from aprilsam_amd import datasets
from tests.support.consumer_graphs import three_components, two_components
from tests.support.mf_emulator import PlanView
import tests.test_gpu_parity as T

# (s and u are multiples of 3 -- three unknowns per pose -- so of "exactly 16, 32 or 48" only 48 can occur: a front of 16 poses,
# three full 16-row blocks of k_selinv_trinv and nothing behind them)
CLASSES = {
    "s < 16": lambda s, u, ch: s < 16,
    "s exactly 16, 32 or 48": lambda s, u, ch: np.isin(s, (16, 32, 48)),
    "s > 64, s mod 16 != 0": lambda s, u, ch: (s > 64) & (s % 16 != 0),
    "u = 0": lambda s, u, ch: u == 0,
    "u < 16": lambda s, u, ch: (u > 0) & (u < 16),
    "u > 64, u mod 16 != 0": lambda s, u, ch: (u > 64) & (u % 16 != 0),
    "more than 1 000 children": lambda s, u, ch: ch > 1000,
}


def _graphs(lib):
    return {"random 700/600/21": datasets.random_pose_graph(700, 600, 21), "random 3000/1800/102": datasets.random_pose_graph(3000, 1800, 102),
            "lattice 60": lib.lattice_arrays(60), "two components": two_components()[0], "three components": three_components()[0],
            "star 3000": T._star(3000, 1), "star 70": T._star(70, 2), "chain 4000": T._chain(4000, 3)}


def test_the_consumer_graphs_cover_every_front_shape_class(lib):
    counts = {}
    for name, arr in _graphs(lib).items():
        P = PlanView(lib, len(arr[0]), arr[1], arr[2], xy=arr[0][:, :2])
        s, u, ch = 3 * P.front_nsb, 3 * P.front_nub, np.diff(P.ch_ptr)
        counts[name] = {c: int(np.sum(f(s, u, ch))) for c, f in CLASSES.items()}
        counts[name]["fronts"] = P.nF
    cols = ["fronts"] + list(CLASSES)
    print("\n" + " | ".join(["graph".ljust(22)] + cols))
    for name, row in counts.items():
        print(" | ".join([name.ljust(22)] + [str(row[c]).rjust(len(c)) for c in cols]))
    for c in CLASSES:
        assert sum(row[c] for row in counts.values()) > 0, c
    # several roots: u = 0 on more than one front of ONE graph
    assert counts["two components"]["u = 0"] >= 2 and counts["three components"]["u = 0"] >= 3
    assert counts["random 3000/1800/102"]["s > 64, s mod 16 != 0"] > 0          # (the root front: 645 poses)
