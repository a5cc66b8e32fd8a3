"""`.graph` files (aprilsam/april_graph.c:250-326,377-426 over common/stype.c:75-169).
The reference ships data/M3500.graph = its demo's load of data/M3500.txt saved straight away; the committed M3500
fixture + the demo's "odom"/"scan" tagging rule must therefore serialise to exactly those bytes."""
import hashlib
import os

import numpy as np
import pytest

from aprilsam_amd import datasets

REF_M3500_GRAPH_SHA256 = "e22bbcfe784b179c78de7dee6f803cbdcfb14ee4e7a035e273a9ca1cdf5045c6"     # sha256 of /root/reference/data/M3500.graph
REF_M3500_GRAPH_BYTES = 1820188
REFDATA = "/root/reference/data/M3500.graph"


def _m3500_loaded_graph(lib):
    st, fa, fb, z, W = datasets.m3500_arrays()
    g = lib.new_graph(); g.build_from_arrays(st, fa, fb, z, W)
    for i in range(g.n_factors):
        g.factor_attr_put(i, "type", "odom" if abs(int(fb[i]) - int(fa[i])) == 1 else "scan")      # examples/aprilsam_demo.c:83-87
    return g


def test_writer_reproduces_the_reference_data_file_byte_for_byte(lib, tmp_path):
    g = _m3500_loaded_graph(lib)
    path = str(tmp_path / "m3500.graph")
    assert g.save(path)
    data = open(path, "rb").read()
    assert len(data) == REF_M3500_GRAPH_BYTES and hashlib.sha256(data).hexdigest() == REF_M3500_GRAPH_SHA256
    if os.path.exists(REFDATA):                                   # belt and braces where the reference tree is mounted
        assert data == open(REFDATA, "rb").read()
    g.destroy()


def test_round_trip_keeps_numbers_structure_and_string_attributes(lib, tmp_path):
    st, fa, fb, z, W = datasets.random_pose_graph(60, 40, seed=3)           # includes an xytpos prior and full W matrices
    g = lib.new_graph(); g.build_from_arrays(st, fa, fb, z, W)
    g.factor_attr_put(2, "type", "scan"); g.factor_attr_put(2, "note", "second key"); g.factor_attr_put(2, "type", "odom")
    path = str(tmp_path / "r.graph")
    assert g.save(path, magic_offset=12345)
    h = lib.load_graph(path)
    a, b = g.arrays(), h.arrays()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert h.factor_attr_get(2, "type") == "odom" and h.factor_attr_get(2, "note") == "second key" and h.factor_attr_get(3, "type") is None
    # a second generation is identical to the first (same magic start)
    path2 = str(tmp_path / "r2.graph")
    assert h.save(path2, magic_offset=12345) and open(path, "rb").read() == open(path2, "rb").read()
    g.destroy(); h.destroy()


def test_reader_rejects_garbage_and_truncation(lib, tmp_path):
    assert lib.load_graph(str(tmp_path / "missing.graph")) is None
    bad = tmp_path / "bad.graph"; bad.write_bytes(b"not a graph file at all, just text")
    assert lib.load_graph(str(bad)) is None
    g = lib.new_graph(); g.build_from_arrays(*datasets.random_pose_graph(8, 3, seed=1))
    ok = str(tmp_path / "ok.graph"); assert g.save(ok)
    data = open(ok, "rb").read()
    cut = tmp_path / "cut.graph"; cut.write_bytes(data[: len(data) // 2])
    assert lib.load_graph(str(cut)) is None
    flip = bytearray(data); flip[-3] ^= 0xFF                              # trailing magic no longer matches
    bad2 = tmp_path / "flip.graph"; bad2.write_bytes(bytes(flip))
    assert lib.load_graph(str(bad2)) is None
    g.destroy()


def test_interchange_with_the_live_reference(lib, reflib, tmp_path):
    """our files load in the reference, the reference's files load here (needs oracle/_ref)"""
    if not hasattr(reflib.dll, "stype_register_basic_types"):
        pytest.skip("reference build without the serialisation sources")
    arrays = datasets.random_pose_graph(30, 20, seed=7)
    ours = lib.new_graph(); ours.build_from_arrays(*arrays)
    p1 = str(tmp_path / "ours.graph"); assert ours.save(p1)
    rg = reflib.load_graph(p1)
    assert rg is not None
    for x, y in zip(ours.arrays(), rg.arrays()):
        assert np.array_equal(x, y)
    p2 = str(tmp_path / "ref.graph"); assert rg.save(p2)
    back = lib.load_graph(p2)
    for x, y in zip(ours.arrays(), back.arrays()):
        assert np.array_equal(x, y)
    ours.destroy(); back.destroy()


def test_reader_loads_the_reference_data_file(lib, tmp_path):
    """the reference's data/M3500.graph, byte for byte: rebuilt from the committed fixture by the writer and pinned by its sha256"""
    g = _m3500_loaded_graph(lib)
    path = str(tmp_path / "M3500.graph")
    assert g.save(path)
    g.destroy()
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == REF_M3500_GRAPH_SHA256
    g = lib.load_graph(path)
    st, fa, fb, z, W = datasets.m3500_arrays()
    a = g.arrays()
    assert np.array_equal(a[0], st) and np.array_equal(a[1], fa) and np.array_equal(a[2], fb) and np.array_equal(a[3], z) and np.array_equal(a[4], W)
    assert g.factor_attr_get(0, "type") in ("odom", "scan")
    g.destroy()
