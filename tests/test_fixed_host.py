"""Fixed nodes, host side: aprilsam_amd_node_set_fixed / _get_fixed -- the round trip, the deep copy, destroy
after set and after set-and-clear, every refusal (a foreign pointer in node->impl included), and .graph files, which do not store the
flag.  No GPU."""
import ctypes as C

import numpy as np

from aprilsam_amd import abi

_COPY = C.CFUNCTYPE(C.POINTER(abi.Node), C.c_void_p)
_DESTROY = C.CFUNCTYPE(None, C.c_void_p)


def _node(lib, state=(1.0, 2.0, 0.5)):
    s = (C.c_double * 3)(*state)
    return lib.dll.april_graph_node_xyt_create(s, s, s)


def _destroy(n):
    _DESTROY(n.contents.destroy)(C.cast(n, C.c_void_p))


def _copy(n):
    return _COPY(n.contents.copy)(C.cast(n, C.c_void_p))


def test_round_trip(lib):
    d = lib.dll
    n = _node(lib)
    assert not n.contents.impl and d.aprilsam_amd_node_get_fixed(n) == 0
    assert d.aprilsam_amd_node_set_fixed(n, 1) == 0 and n.contents.impl and d.aprilsam_amd_node_get_fixed(n) == 1
    blk = n.contents.impl
    assert d.aprilsam_amd_node_set_fixed(n, 1) == 0 and n.contents.impl == blk          # (fixing twice keeps the one block)
    assert d.aprilsam_amd_node_set_fixed(n, 0) == 0 and not n.contents.impl and d.aprilsam_amd_node_get_fixed(n) == 0
    assert d.aprilsam_amd_node_set_fixed(n, 0) == 0 and not n.contents.impl             # (freeing a free node)
    _destroy(n)                                                                          # destroy after set and clear


def test_copy_is_deep_and_destroy_frees_the_block(lib):
    d = lib.dll
    n = _node(lib)
    assert d.aprilsam_amd_node_set_fixed(n, 1) == 0
    c = _copy(n)
    assert c.contents.impl and c.contents.impl != n.contents.impl and d.aprilsam_amd_node_get_fixed(c) == 1
    assert [c.contents.state[k] for k in range(3)] == [1.0, 2.0, 0.5]
    assert d.aprilsam_amd_node_set_fixed(n, 0) == 0
    assert d.aprilsam_amd_node_get_fixed(c) == 1 and d.aprilsam_amd_node_get_fixed(n) == 0   # each owns its flag
    c2 = _copy(n)
    assert not c2.contents.impl
    _destroy(c)                                                                          # destroy after set
    _destroy(c2); _destroy(n)


def test_refusals(lib):
    d = lib.dll
    lib.clear_error()
    assert d.aprilsam_amd_node_set_fixed(None, 1) == -13 and lib.last_error()[0] == -13
    assert d.aprilsam_amd_node_get_fixed(None) == 0
    n = _node(lib)
    for bad in (2, -1, 7):
        lib.clear_error()
        assert d.aprilsam_amd_node_set_fixed(n, bad) == -13 and lib.last_error()[0] == -13 and not n.contents.impl
    # node->impl in use by something that is not this library's block
    foreign = (C.c_ulonglong * 2)(0x1234, 0)
    n.contents.impl = C.addressof(foreign)
    for v in (1, 0):
        lib.clear_error()
        assert d.aprilsam_amd_node_set_fixed(n, v) == -12
        code, msg = lib.last_error()
        assert code == -12 and "impl" in msg and n.contents.impl == C.addressof(foreign)
    assert d.aprilsam_amd_node_get_fixed(n) == 0
    n.contents.impl = None
    # not an xyt node
    n.contents.type = 7
    lib.clear_error()
    assert d.aprilsam_amd_node_set_fixed(n, 1) == -12 and lib.last_error()[0] == -12 and not n.contents.impl
    assert d.aprilsam_amd_node_get_fixed(n) == 0
    n.contents.type = 100
    assert d.aprilsam_amd_node_set_fixed(n, 1) == 0
    _destroy(n)


def test_graph_wrappers_and_destroy(lib):
    g = lib.new_graph()
    for i in range(5):
        g.add_node_xyt([float(i), 0.0, 0.0])
    assert [g.get_fixed(i) for i in range(5)] == [False] * 5
    assert g.set_fixed(0) == 0 and g.set_fixed(3, True) == 0 and g.set_fixed(4, 1) == 0 and g.set_fixed(4, False) == 0
    assert [g.get_fixed(i) for i in range(5)] == [True, False, False, True, False]
    assert g.set_fixed(1, 2) == -13
    g.destroy()                                                                          # fixed nodes die with their graph


def test_graph_files_do_not_store_the_flag(lib, tmp_path):
    g = lib.new_graph()
    for i in range(4):
        g.add_node_xyt([float(i), 0.5 * i, 0.1 * i])
    for i in range(3):
        g.add_factor_xyt(i, i + 1, [1.0, 0.5, 0.1], np.eye(3))
    g.add_factor_xytpos(0, [0.0, 0.0, 0.0], np.eye(3))
    assert g.set_fixed(0) == 0 and g.set_fixed(2) == 0
    path = tmp_path / "fixed.graph"
    assert g.save(str(path)) is True                      # save ignores the flag ...
    plain = lib.new_graph()
    for i in range(4):
        plain.add_node_xyt([float(i), 0.5 * i, 0.1 * i])
    for i in range(3):
        plain.add_factor_xyt(i, i + 1, [1.0, 0.5, 0.1], np.eye(3))
    plain.add_factor_xytpos(0, [0.0, 0.0, 0.0], np.eye(3))
    path2 = tmp_path / "plain.graph"
    assert plain.save(str(path2)) is True
    assert path.read_bytes() == path2.read_bytes()        # ... the file is the free graph's, byte for byte
    h = lib.load_graph(str(path))
    assert h is not None and h.n_nodes == 4
    assert [h.get_fixed(i) for i in range(4)] == [False] * 4     # ... and load returns free nodes
    assert np.array_equal(h.states(), g.states())
    assert [g.get_fixed(i) for i in range(4)] == [True, False, True, False]
    for x in (g, plain, h):
        x.destroy()
