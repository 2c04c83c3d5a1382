"""Host-side checks of the per-graph readouts (reduce_nodes / reduce_edges / softmax_nodes / softmax_edges / broadcast_nodes /
broadcast_edges / graph_indicator, /root/reference/src/NeuralGraphPDE.jl:5-7): the exported names, the argument checks the library
makes before any device call, and the bookkeeping of the graph indicator through the constructor, copies and batch().  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib

NAMES = ["reduce_nodes", "reduce_edges", "softmax_nodes", "softmax_edges", "broadcast_nodes", "broadcast_edges", "graph_indicator"]


def test_names_are_exported():
    for name in NAMES:
        assert name in ng.__all__, name
        assert callable(getattr(ng, name)), name


def entries(lib):
    """(name, call with plan = NULL, width d, aggregation aggr) for every entry that takes a plan"""
    return [
        ("reduce_forward", lambda d, a: lib.ngpde_readout_reduce_forward(None, d, a, None, None, None, 0, None), True),
        ("reduce_backward", lambda d, a: lib.ngpde_readout_reduce_backward(None, d, a, None, None, None, None, None), True),
        ("softmax_forward", lambda d, a: lib.ngpde_readout_softmax_forward(None, d, None, None, None, 0, None), False),
        ("softmax_backward", lambda d, a: lib.ngpde_readout_softmax_backward(None, d, None, None, None, None, 0, None), False),
        ("broadcast_forward", lambda d, a: lib.ngpde_readout_broadcast_forward(None, d, None, None, None), False),
        ("broadcast_backward", lambda d, a: lib.ngpde_readout_broadcast_backward(None, d, None, None, None, 0, None), False),
    ]


def test_null_plan_is_refused():
    lib = _lib.load()
    for name, call, _ in entries(lib):
        assert call(4, _lib.AGGR["+"]) == _lib.ERR_INVALID_ARGUMENT, name
        assert b"readout is NULL" in lib.ngpde_last_error(), name
    assert lib.ngpde_readout_info(None, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.ngpde_readout_workspace_bytes(None, 64) == 0


def test_negative_width_is_refused_first():
    lib = _lib.load()
    for name, call, _ in entries(lib):
        assert call(-1, _lib.AGGR["*"]) == _lib.ERR_DIMENSION_MISMATCH, name      # before the aggregation and the NULL plan
        assert b"negative width" in lib.ngpde_last_error(), name


def test_mul_is_refused():
    lib = _lib.load()
    for name, call, takes_aggr in entries(lib):
        if takes_aggr:
            for bad in (_lib.AGGR["*"], 5, -1):
                assert call(4, bad) == _lib.ERR_INVALID_ARGUMENT, (name, bad)
                assert b"aggregation" in lib.ngpde_last_error(), (name, bad)         # (not the NULL plan: checked after)
    g = ng.GNNGraph([1, 1, 2, 3], [2, 3, 1, 1], num_nodes=3)
    x = np.ones((2, 3), dtype=np.float32)
    for aggr in ("*", "mul", "prod", "median", None):
        with pytest.raises(ng.ArgumentError):
            ng.reduce_nodes(aggr, g, x)
        with pytest.raises(ng.ArgumentError):
            ng.reduce_edges(aggr, g, np.ones((2, 4), dtype=np.float32))


def test_create_refuses_bad_segment_counts_without_a_device():
    lib = _lib.load()
    out = C.c_void_p()
    assert lib.ngpde_readout_create(10, None, None, 0, 0, None, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT and not out.value
    assert b"n_segments" in lib.ngpde_last_error()
    assert lib.ngpde_readout_create(10, None, None, 0, 3, None, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT and not out.value
    assert b"graph_indicator" in lib.ngpde_last_error()
    assert lib.ngpde_readout_create(-1, None, None, 0, 1, None, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT and not out.value


def test_destroy_null():
    assert _lib.load().ngpde_readout_destroy(None) == 0


# ---- the indicator on the host ----------------------------------------------------------------------------------------------------


def check_indicator(g, gi0):
    """gi0: the expected 0-based graph id per node"""
    gi0 = np.asarray(gi0)
    assert np.array_equal(ng.graph_indicator(g), gi0 + 1)
    s0 = g.edge_index(index_base=0)[0]
    assert np.array_equal(ng.graph_indicator(g, edges=True), gi0[s0] + 1)
    assert np.array_equal(ng.graph_indicator(g, edges=False), gi0 + 1)
    if g.num_graphs == 1:
        assert g.graph_indicator is None
    else:
        assert g.graph_indicator.dtype == np.int32 and np.array_equal(g.graph_indicator, gi0)


@pytest.mark.parametrize("base", [0, 1])
def test_constructor_honours_index_base(base):
    s0, t0 = np.array([0, 1, 2, 3, 4, 4]), np.array([1, 0, 3, 2, 5, 4])
    gi0 = np.array([0, 0, 1, 1, 2, 2])
    g = ng.GNNGraph(s0 + base, t0 + base, num_nodes=6, index_base=base, graph_indicator=gi0 + base)
    assert g.num_graphs == 3
    check_indicator(g, gi0)
    g4 = ng.GNNGraph(s0 + base, t0 + base, num_nodes=6, index_base=base, graph_indicator=gi0 + base, num_graphs=4)   # graph 4 is empty
    assert g4.num_graphs == 4
    check_indicator(g4, gi0)
    with pytest.raises(ng.DimensionMismatch):
        ng.GNNGraph(s0 + base, t0 + base, num_nodes=6, index_base=base, graph_indicator=gi0[:5] + base)
    with pytest.raises(ng.ArgumentError):
        ng.GNNGraph(s0 + base, t0 + base, num_nodes=6, index_base=base, graph_indicator=gi0 + base, num_graphs=2)


def test_single_graph_is_all_ones():
    g = ng.GNNGraph([1, 1, 2, 3], [2, 3, 1, 1], num_nodes=3)           # test/runtests.jl:11-13
    check_indicator(g, np.zeros(3, dtype=np.int64))
    assert ng.graph_indicator(g, edges=True).shape == (4,)


def test_copy_constructor_shares_the_indicator():
    gi0 = np.array([1, 0, 1, 0, 2])                                     # (not sorted: any map is kept as given)
    g = ng.GNNGraph([0, 1, 2], [2, 3, 0], num_nodes=5, index_base=0, graph_indicator=gi0)
    for c in (ng.GNNGraph(g), g.copy(ndata=np.zeros((2, 5), dtype=np.float32))):
        assert c.graph_indicator is g.graph_indicator and c.num_graphs == 3
        check_indicator(c, gi0)


def members():
    rng = np.random.default_rng(3)
    out = []
    for n, e in ((4, 6), (1, 0), (9, 20)):
        out.append(ng.GNNGraph(rng.integers(0, n, e), rng.integers(0, n, e), num_nodes=n, index_base=0))
    return out


def test_batch_concatenates_indicators():
    gs = members()
    b = ng.batch(gs)
    assert b.num_graphs == 3
    check_indicator(b, np.repeat([0, 1, 2], [4, 1, 9]))


def test_batch_of_a_batch_offsets_by_graphs():
    gs = members()
    inner = ng.batch(gs[:2])
    shuffled = ng.GNNGraph([0, 2], [1, 3], num_nodes=4, index_base=0, graph_indicator=[1, 0, 1, 0])
    b = ng.batch([gs[2], inner, shuffled, gs[1]])
    assert b.num_graphs == 1 + 2 + 2 + 1
    check_indicator(b, np.concatenate([np.zeros(9, int), np.repeat([1, 2], [4, 1]), np.array([4, 3, 4, 3]), [5]]))


def test_many_graphs_without_an_indicator_are_refused():
    g = ng.GNNGraph([0, 1, 2], [1, 0, 3], num_nodes=4, index_base=0, num_graphs=2)     # what a padded batch looks like
    assert g.graph_indicator is None
    with pytest.raises(ng.ArgumentError, match="graph_indicator"):
        ng.graph_indicator(g)
    with pytest.raises(ng.ArgumentError, match="padded batch"):
        ng.reduce_nodes("+", g, np.ones((2, 4), dtype=np.float32))
    with pytest.raises(ng.ArgumentError, match="padded batch"):
        ng.broadcast_edges(g, np.ones((2, 2), dtype=np.float32))
    assert ng.batch([g, g]).graph_indicator is None
