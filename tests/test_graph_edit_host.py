"""Host-side checks of the graph editing and negative sampling (editing.py over csrc/graph_edit.hip; src/NeuralGraphPDE.jl:4 of the
reference re-exports add_nodes, add_edges, remove_edges, remove_nodes, to_unidirected, set_edge_weight, get_edge_weight and
negative_sample from GNNGraphs): the exported names, the argument errors the package raises before any device call, and what the five
new C entries refuse before they touch the device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib

NAMES = ("add_nodes", "add_edges", "remove_edges", "remove_nodes", "to_unidirected", "set_edge_weight", "get_edge_weight", "negative_sample")


def graph(**kw):
    return ng.GNNGraph([0, 0, 1, 2], [1, 2, 0, 0], num_nodes=3, index_base=0, **kw)


def test_names_are_exported():
    for name in NAMES:
        assert name in ng.__all__, name
        assert callable(getattr(ng, name)), name


def test_add_nodes_argument_errors():
    for n in (-1, -7, 1.5, "2", None, True):
        with pytest.raises(ng.ArgumentError, match="n must be"):
            ng.add_nodes(graph(), n)
    g = graph(ndata={"x": np.zeros((2, 3), np.float32), "y": np.zeros(3, np.int64)})
    for ndata in (None, {"x": np.zeros((2, 2), np.float32)}, {"x": np.zeros((2, 2), np.float32), "z": np.zeros(2, np.int64)},
                  np.zeros((2, 2), np.float32)):
        with pytest.raises(ng.ArgumentError, match="same keys"):
            ng.add_nodes(g, 2, ndata)
    with pytest.raises(ng.ArgumentError, match="last dimension must be 2"):
        ng.add_nodes(g, 2, {"x": np.zeros((2, 3), np.float32), "y": np.zeros(2, np.int64)})
    with pytest.raises(ng.ArgumentError, match="same keys"):
        ng.add_nodes(graph(), 2, {"x": np.zeros((2, 2), np.float32)})          # features for a graph that has none
    gb = ng.GNNGraph([0, 2], [1, 3], num_nodes=4, index_base=0, graph_indicator=[0, 0, 1, 1])
    with pytest.raises(ng.ArgumentError, match="batch"):
        ng.add_nodes(gb, 1)


def test_add_edges_argument_errors():
    g = graph(edata={"e": np.zeros((2, 4), np.float32)})
    for edata in (None, {"f": np.zeros((2, 1), np.float32)}):
        with pytest.raises(ng.ArgumentError, match="same keys"):
            ng.add_edges(g, [0], [1], edata)
    with pytest.raises(ng.ArgumentError, match="last dimension must be 1"):
        ng.add_edges(g, [0], [1], np.zeros((2, 2), np.float32))
    with pytest.raises(ng.DimensionMismatch):
        ng.add_edges(g, [0], [1], np.zeros((3, 1), np.float32))
    with pytest.raises(ng.DimensionMismatch):
        ng.add_edges(graph(), [0, 1], [1])
    gw = graph(edge_weight=np.ones(4, np.float32))
    with pytest.raises(ng.ArgumentError, match="edge_weight"):
        ng.add_edges(gw, [0], [1])
    with pytest.raises(ng.ArgumentError, match="edge_weight"):
        ng.add_edges(graph(), [0], [1], edge_weight=np.ones(1, np.float32))
    with pytest.raises(ng.ArgumentError, match="edge_weight"):
        ng.add_edges(gw, [0], [1], edge_weight=np.ones(2, np.float32))


def test_edge_weight_accessors():
    g = graph()
    assert ng.get_edge_weight(g) is None
    w = np.arange(4, dtype=np.float32)
    gw = ng.set_edge_weight(g, w)
    assert ng.get_edge_weight(gw) is w and ng.get_edge_weight(g) is None and gw == g
    for bad in (np.ones(3, np.float32), np.ones(5, np.float32), None):
        with pytest.raises(ng.DimensionMismatch):
            ng.set_edge_weight(g, bad)


def test_negative_sample_argument_errors():
    for num in (-1, 2.0, "3", True, [1]):
        with pytest.raises(ng.ArgumentError, match="num_neg_edges"):
            ng.negative_sample(graph(), num)
    for seed in (1.5, "7", [1], True, -1, 2 ** 64):
        with pytest.raises(ng.ArgumentError, match="seed"):
            ng.negative_sample(graph(), 2, seed=seed)
        with pytest.raises(ng.ArgumentError, match="seed"):
            ng.negative_sample(graph(), seed=seed, bidirected=False)


# ---- the C entries --------------------------------------------------------------------------------------------------------------

ONE = C.c_void_p(16)     # (never dereferenced: the checks come before any device call)


def append(lib, n=3, e=4, s=ONE, t=ONE, n_new=2, new=(ONE, ONE), outs=(ONE, ONE)):
    return lib.ngpde_coo_append(n, e, s, t, 0, n_new, new[0], new[1], None, outs[0], outs[1], None)


def remove(lib, n=3, e=4, s=ONE, t=ONE, n_listed=2, positions=ONE, pairs=(None, None), outs=(ONE, ONE, ONE), n_out=True):
    n64 = C.c_int64(7)
    st = lib.ngpde_coo_remove_edges(n, e, s, t, 0, n_listed, positions, pairs[0], pairs[1], outs[0], outs[1], outs[2],
                                    C.byref(n64) if n_out else None, None)
    return st, n64.value


def complement(lib, n=3, n_listed=2, nodes=ONE, out=ONE, n_out=True):
    n64 = C.c_int64(7)
    st = lib.ngpde_coo_complement_nodes(n, n_listed, nodes, out, C.byref(n64) if n_out else None, None)
    return st, n64.value


def orient(lib, n=3, e=4, s=ONE, t=ONE, outs=(ONE, ONE)):
    return lib.ngpde_coo_orient(n, e, s, t, outs[0], outs[1], None)


def negative(lib, n=3, e=4, s=ONE, t=ONE, n_target=2, bidirected=0, chunk=0, outs=(ONE, ONE), n_out=True):
    n64 = C.c_int64(7)
    st = lib.ngpde_coo_negative_sample(n, e, s, t, 0, n_target, bidirected, 5, chunk, outs[0], outs[1], C.byref(n64) if n_out else None, None)
    return st, n64.value


def status(r):
    return r[0] if isinstance(r, tuple) else r


def test_coo_entries_refuse_null_and_negative_arguments():
    lib = _lib.load()
    for name, call in (("ngpde_coo_append", append), ("ngpde_coo_remove_edges", remove), ("ngpde_coo_orient", orient),
                       ("ngpde_coo_negative_sample", negative)):
        assert status(call(lib, s=None, t=None)) == _lib.ERR_INVALID_ARGUMENT, name
        msg = lib.ngpde_last_error()
        assert b"NULL" in msg and name.encode() in msg, (name, msg)
        for n, e in ((-1, 0), (3, -1)):
            assert status(call(lib, n=n, e=e)) == _lib.ERR_INVALID_ARGUMENT, name
            assert b"negative" in lib.ngpde_last_error(), name
        assert status(call(lib, e=2 ** 31)) == _lib.ERR_INVALID_ARGUMENT and b"2^31" in lib.ngpde_last_error(), name
        assert status(call(lib, n=2 ** 31, e=0)) == _lib.ERR_INVALID_ARGUMENT and b"2^31" in lib.ngpde_last_error(), name
        assert status(call(lib, n=0, e=4)) == _lib.ERR_DIMENSION_MISMATCH, name
        for k in range(2):
            outs = [ONE, ONE, ONE][:3 if call is remove else 2]
            outs[k] = None
            assert status(call(lib, outs=tuple(outs))) == _lib.ERR_INVALID_ARGUMENT and b"is NULL" in lib.ngpde_last_error(), name
    for call in (remove, negative):
        st, count = call(lib, n_out=False)
        assert st == _lib.ERR_INVALID_ARGUMENT and b"n_out is NULL" in lib.ngpde_last_error()
        assert call(lib, s=None, t=None)[1] in (0, 7)


def test_append_checks():
    lib = _lib.load()
    assert append(lib, n_new=-1) == _lib.ERR_INVALID_ARGUMENT and b"negative" in lib.ngpde_last_error()
    assert append(lib, new=(None, ONE)) == _lib.ERR_INVALID_ARGUMENT and b"s_new / t_new is NULL" in lib.ngpde_last_error()
    assert append(lib, new=(ONE, None)) == _lib.ERR_INVALID_ARGUMENT and b"s_new / t_new is NULL" in lib.ngpde_last_error()
    assert append(lib, e=2 ** 31 - 2, n_new=2) == _lib.ERR_INVALID_ARGUMENT and b"after the append" in lib.ngpde_last_error()
    assert append(lib, n=0, e=0, s=None, t=None, n_new=1) == _lib.ERR_DIMENSION_MISMATCH
    assert append(lib, e=0, s=None, t=None, n_new=0, new=(None, None), outs=(None, None)) == 0          # nothing to do is not an error


def test_remove_edges_checks():
    lib = _lib.load()
    assert remove(lib, n_listed=-1)[0] == _lib.ERR_INVALID_ARGUMENT and b"n_listed" in lib.ngpde_last_error()
    assert remove(lib, n_listed=2 ** 31)[0] == _lib.ERR_INVALID_ARGUMENT and b"n_listed" in lib.ngpde_last_error()
    assert remove(lib, positions=None)[0] == _lib.ERR_INVALID_ARGUMENT and b"list is NULL" in lib.ngpde_last_error()
    assert remove(lib, pairs=(ONE, ONE))[0] == _lib.ERR_INVALID_ARGUMENT and b"both positions and pairs" in lib.ngpde_last_error()
    for pairs in ((ONE, None), (None, ONE)):
        assert remove(lib, positions=None, pairs=pairs)[0] == _lib.ERR_INVALID_ARGUMENT and b"one of ls / lt" in lib.ngpde_last_error()
    assert remove(lib, outs=(ONE, ONE, None))[0] == _lib.ERR_INVALID_ARGUMENT and b"output is NULL" in lib.ngpde_last_error()
    assert remove(lib, n=0, e=0, s=None, t=None, positions=None, pairs=(ONE, ONE), outs=(None, None, None))[0] == _lib.ERR_INVALID_ARGUMENT


def test_complement_nodes_checks():
    lib = _lib.load()
    for n, n_listed in ((-1, 0), (3, -1)):
        assert complement(lib, n=n, n_listed=n_listed)[0] == _lib.ERR_INVALID_ARGUMENT and b"negative" in lib.ngpde_last_error()
    for n, n_listed in ((2 ** 31, 0), (3, 2 ** 31)):
        assert complement(lib, n=n, n_listed=n_listed)[0] == _lib.ERR_INVALID_ARGUMENT and b"2^31" in lib.ngpde_last_error()
    assert complement(lib, n_out=False)[0] == _lib.ERR_INVALID_ARGUMENT and b"n_out is NULL" in lib.ngpde_last_error()
    assert complement(lib, nodes=None) == (_lib.ERR_INVALID_ARGUMENT, 0) and b"nodes is NULL" in lib.ngpde_last_error()
    assert complement(lib, out=None) == (_lib.ERR_INVALID_ARGUMENT, 0) and b"out is NULL" in lib.ngpde_last_error()
    assert complement(lib, n=0, n_listed=0, nodes=None, out=None) == (0, 0)          # nothing to do is not an error


def test_orient_and_negative_sample_checks():
    lib = _lib.load()
    assert orient(lib, e=0, s=None, t=None, outs=(None, None)) == 0
    for n_target in (-1, 2 ** 31):
        assert negative(lib, n_target=n_target)[0] == _lib.ERR_INVALID_ARGUMENT and b"n_target" in lib.ngpde_last_error()
    assert negative(lib, n_target=2 ** 30, bidirected=1)[0] == _lib.ERR_INVALID_ARGUMENT and b"n_target" in lib.ngpde_last_error()
    for chunk in (-1, 2 ** 24 + 1):
        assert negative(lib, chunk=chunk)[0] == _lib.ERR_INVALID_ARGUMENT and b"chunk" in lib.ngpde_last_error()
    # more negatives than the nodes have pairs: known without the device (3 nodes: 6 ordered pairs, 3 unordered)
    assert negative(lib, n_target=7) == (_lib.ERR_INVALID_ARGUMENT, 0) and b"pairs" in lib.ngpde_last_error()
    assert negative(lib, n_target=4, bidirected=1) == (_lib.ERR_INVALID_ARGUMENT, 0) and b"pairs" in lib.ngpde_last_error()
    assert negative(lib, n=1, e=0, s=None, t=None, n_target=1) == (_lib.ERR_INVALID_ARGUMENT, 0)
    assert negative(lib, n_target=0, outs=(None, None)) == (0, 0)          # nothing to do is not an error
