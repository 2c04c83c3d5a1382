"""Host-side checks of the graph queries and transforms (degree, has_self_loops, has_multi_edges, is_bidirected, add_self_loops,
remove_self_loops, remove_multi_edges, to_bidirected, induced_subgraph, getgraph, unbatch; src/NeuralGraphPDE.jl:4 of the reference
re-exports them from GNNGraphs): the exported names, the argument errors the package raises before any device call, and what every new
C entry refuses before it touches the device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib

NAMES = ["degree", "has_self_loops", "has_multi_edges", "is_bidirected", "add_self_loops", "remove_self_loops", "remove_multi_edges",
         "to_bidirected", "induced_subgraph", "getgraph", "unbatch"]


def test_names_are_exported():
    for name in NAMES:
        assert name in ng.__all__, name
        assert callable(getattr(ng, name)), name


def graph(**kw):
    return ng.GNNGraph([0, 0, 1, 2], [1, 2, 0, 0], num_nodes=3, index_base=0, **kw)


def test_unknown_aggr_is_refused():
    g = graph(edata=np.ones((2, 4), dtype=np.float32))
    for aggr in ("*", "prod", "median", None, 3):
        with pytest.raises(ng.ArgumentError, match="aggregation"):
            ng.remove_multi_edges(g, aggr)
        with pytest.raises(ng.ArgumentError, match="aggregation"):
            ng.remove_multi_edges(g, aggr=aggr)


def test_unknown_dir_is_refused():
    for dir in ("inout", "IN", None, 0):
        with pytest.raises(ng.ArgumentError, match="dir"):
            ng.degree(graph(), dir)
        with pytest.raises(ng.ArgumentError, match="dir"):
            ng.degree(graph(), dir=dir, edge_weight=False)


def test_add_self_loops_refuses_edge_features():
    with pytest.raises(ng.ArgumentError, match="edata"):
        ng.add_self_loops(graph(edata=np.ones((2, 4), dtype=np.float32)))


def test_reducing_an_integer_feature_is_refused():
    g = graph(edata={"e": np.ones((2, 4), dtype=np.float32), "label": np.arange(4)})
    with pytest.raises(ng.ArgumentError, match="label"):
        ng.remove_multi_edges(g)
    with pytest.raises(ng.ArgumentError, match="label"):
        ng.to_bidirected(g)
    with pytest.raises(ng.ArgumentError, match="edge_weight"):
        ng.to_bidirected(graph(edge_weight=np.arange(4)))


def test_getgraph_refuses_bad_positions():
    gb = ng.batch([graph(), graph(), graph()])
    assert gb.num_graphs == 3
    for bad in (3, -1, [0, 3], [1, 1], [2, 0], [], 1.5, [0.5], "a", None):
        with pytest.raises(ng.ArgumentError, match="getgraph"):
            ng.getgraph(gb, bad)
    with pytest.raises(ng.ArgumentError, match="getgraph"):
        ng.getgraph(graph(), 1)            # a single graph has position 0 only


def test_many_graphs_without_an_indicator_are_refused():
    g = ng.GNNGraph([0, 1, 2], [1, 0, 3], num_nodes=4, index_base=0, num_graphs=2)
    assert g.graph_indicator is None
    with pytest.raises(ng.ArgumentError, match="graph_indicator"):
        ng.getgraph(g, 0)
    with pytest.raises(ng.ArgumentError, match="graph_indicator"):
        ng.unbatch(g)


# ---- the C entries --------------------------------------------------------------------------------------------------------------


def entries(lib):
    """(name, call(n_nodes, n_edges) with every pointer NULL)"""
    n64, i32 = C.c_int64(0), C.c_int32(0)
    return [
        ("ngpde_coo_degree", lambda n, e: lib.ngpde_coo_degree(n, e, None, None, 0, 0, None, None, None, None)),
        ("ngpde_coo_flags", lambda n, e: lib.ngpde_coo_flags(n, e, None, None, 0, C.byref(i32), C.byref(i32), C.byref(i32), None)),
        ("ngpde_coo_compact", lambda n, e: lib.ngpde_coo_compact(n, e, None, None, 0, 0, None, 1, None, None, None, C.byref(n64), None)),
        ("ngpde_coo_coalesce", lambda n, e: lib.ngpde_coo_coalesce(n, e, None, None, 0, 0, None, None, None, None, None, C.byref(n64), None)),
        ("ngpde_coo_add_self_loops", lambda n, e: lib.ngpde_coo_add_self_loops(n, e, None, None, 0, None, None, None, None, None)),
    ]


def test_null_coo_lists_are_refused():
    lib = _lib.load()
    for name, call in entries(lib):
        assert call(3, 4) == _lib.ERR_INVALID_ARGUMENT, name
        msg = lib.ngpde_last_error()
        assert b"NULL" in msg and name.encode() in msg, (name, msg)


def test_negative_sizes_are_refused():
    lib = _lib.load()
    for name, call in entries(lib):
        for n, e in ((-1, 0), (3, -1)):
            assert call(n, e) == _lib.ERR_INVALID_ARGUMENT, name
            assert b"negative" in lib.ngpde_last_error(), name


def test_too_many_edges_are_refused():
    lib = _lib.load()
    for name, call in entries(lib):
        assert call(3, 2**31) == _lib.ERR_INVALID_ARGUMENT, name
        assert b"2^31" in lib.ngpde_last_error(), name
    n64 = C.c_int64(0)
    # symmetrising doubles the list: 2^30 edges are 2^31 copies
    assert lib.ngpde_coo_coalesce(3, 2**30, None, None, 0, 1, None, None, None, None, None, C.byref(n64), None) == _lib.ERR_INVALID_ARGUMENT
    assert b"symmetrising" in lib.ngpde_last_error()


def test_null_outputs_are_refused():
    lib = _lib.load()
    one = C.c_void_p(16)     # (never dereferenced: the checks come before any device call)
    n64 = C.c_int64(0)
    assert lib.ngpde_coo_degree(3, 4, one, one, 0, 0, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"output is NULL" in lib.ngpde_last_error()
    assert lib.ngpde_coo_degree(3, 4, one, one, 0, 0, one, one, one, None) == _lib.ERR_INVALID_ARGUMENT      # both forms asked for
    assert b"exactly one" in lib.ngpde_last_error()
    assert lib.ngpde_coo_degree(3, 4, one, one, 0, 0, None, None, one, None) == _lib.ERR_INVALID_ARGUMENT    # sums of no weights
    assert b"without w" in lib.ngpde_last_error()
    assert lib.ngpde_coo_degree(3, 4, one, one, 0, 7, None, one, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"dir" in lib.ngpde_last_error()
    assert lib.ngpde_coo_compact(3, 4, one, one, 0, 0, None, 1, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"n_out is NULL" in lib.ngpde_last_error()
    assert lib.ngpde_coo_compact(3, 4, one, one, 0, 2, None, 0, one, one, one, C.byref(n64), None) == _lib.ERR_INVALID_ARGUMENT
    assert b"nodes is NULL" in lib.ngpde_last_error()
    assert lib.ngpde_coo_compact(3, 4, one, one, 0, 0, None, 1, None, None, None, C.byref(n64), None) == _lib.ERR_INVALID_ARGUMENT
    assert b"output is NULL" in lib.ngpde_last_error()
    assert lib.ngpde_coo_coalesce(3, 4, one, one, 0, 0, one, one, None, one, one, C.byref(n64), None) == _lib.ERR_INVALID_ARGUMENT
    assert b"group_ptr is NULL" in lib.ngpde_last_error()
    assert lib.ngpde_coo_coalesce(3, 4, one, one, 0, 0, one, one, one, one, one, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"n_out is NULL" in lib.ngpde_last_error()
    assert lib.ngpde_coo_add_self_loops(3, 4, one, one, 0, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"s_out" in lib.ngpde_last_error()


def test_group_reduce_checks():
    lib = _lib.load()
    fwd = lambda g, r, d, a: lib.ngpde_group_reduce_forward(g, r, d, a, None, None, None, None, None)
    bwd = lambda g, r, c, d, a: lib.ngpde_group_reduce_backward(g, r, c, d, a, None, None, None, None, None, None, None)
    assert fwd(2, 3, 4, _lib.AGGR["+"]) == _lib.ERR_INVALID_ARGUMENT and b"NULL" in lib.ngpde_last_error()
    assert bwd(2, 3, 1, 4, _lib.AGGR["+"]) == _lib.ERR_INVALID_ARGUMENT and b"NULL" in lib.ngpde_last_error()
    for bad in (_lib.AGGR["*"], 5, -1):
        assert fwd(2, 3, 4, bad) == _lib.ERR_INVALID_ARGUMENT and b"aggregation" in lib.ngpde_last_error()
        assert bwd(2, 3, 1, 4, bad) == _lib.ERR_INVALID_ARGUMENT and b"aggregation" in lib.ngpde_last_error()
    assert fwd(-1, 3, 4, 0) == _lib.ERR_INVALID_ARGUMENT and fwd(2, -3, 4, 0) == _lib.ERR_INVALID_ARGUMENT
    assert fwd(2, 3, -4, 0) == _lib.ERR_INVALID_ARGUMENT and b"negative width" in lib.ngpde_last_error()
    assert bwd(2, 3, 3, 4, 0) == _lib.ERR_INVALID_ARGUMENT and b"copies" in lib.ngpde_last_error()
    assert fwd(0, 0, 4, 0) == 0 and bwd(0, 0, 1, 4, 0) == 0          # nothing to do is not an error
