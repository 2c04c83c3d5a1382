"""The message-passing entries (include/ngpde.h, "the public message-passing API") check their arguments before any device call, and
the package exports the API the reference re-exports (src/NeuralGraphPDE.jl:5-11).  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib

API = ["propagate", "apply_edges", "aggregate_neighbors", "softmax_edge_neighbors", "copy_xj", "copy_xi", "xi_dot_xj", "e_mul_xj",
       "w_mul_xj"]


def test_message_passing_api_is_exported():
    for name in API:
        assert name in ng.__all__ and callable(getattr(ng, name)), name


def tables(n, width):
    vp = (C.c_void_p * n)()
    return vp, (C.c_int32 * n)(*width)


def test_null_graph_is_an_invalid_argument():
    lib = _lib.load()
    vp, w = tables(1, [8])
    calls = {
        "ngpde_gather_forward": lambda: lib.ngpde_gather_forward(None, 1, vp, w, vp, vp, None),
        "ngpde_gather_backward": lambda: lib.ngpde_gather_backward(None, 1, w, vp, vp, vp, None),
        "ngpde_propagate_emul_forward": lambda: lib.ngpde_propagate_emul_forward(None, 8, 1, 0, None, None, None, None),
        "ngpde_propagate_emul_backward": lambda: lib.ngpde_propagate_emul_backward(None, 8, 8, 1, None, None, None, None, None, None),
        "ngpde_apply_edges_dot_forward": lambda: lib.ngpde_apply_edges_dot_forward(None, 8, None, None, None, None),
        "ngpde_apply_edges_dot_backward": lambda: lib.ngpde_apply_edges_dot_backward(None, 8, None, None, None, None, None, None),
        "ngpde_softmax_edge_neighbors_forward": lambda: lib.ngpde_softmax_edge_neighbors_forward(None, 4, None, None, None),
        "ngpde_softmax_edge_neighbors_backward": lambda: lib.ngpde_softmax_edge_neighbors_backward(None, 4, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == _lib.ERR_INVALID_ARGUMENT, name
        assert b"graph is NULL" in lib.ngpde_last_error(), name


def test_negative_width_is_a_dimension_mismatch():
    lib = _lib.load()
    vp, w = tables(2, [8, -1])
    calls = {
        "ngpde_gather_forward": lambda: lib.ngpde_gather_forward(None, 2, vp, w, vp, vp, None),
        "ngpde_gather_backward": lambda: lib.ngpde_gather_backward(None, 2, w, vp, vp, vp, None),
        "ngpde_propagate_emul_forward": lambda: lib.ngpde_propagate_emul_forward(None, -1, 0, 0, None, None, None, None),
        "ngpde_propagate_emul_backward": lambda: lib.ngpde_propagate_emul_backward(None, -3, 0, 1, None, None, None, None, None, None),
        "ngpde_apply_edges_dot_forward": lambda: lib.ngpde_apply_edges_dot_forward(None, -1, None, None, None, None),
        "ngpde_apply_edges_dot_backward": lambda: lib.ngpde_apply_edges_dot_backward(None, -1, None, None, None, None, None, None),
        "ngpde_softmax_edge_neighbors_forward": lambda: lib.ngpde_softmax_edge_neighbors_forward(None, -2, None, None, None),
        "ngpde_softmax_edge_neighbors_backward": lambda: lib.ngpde_softmax_edge_neighbors_backward(None, -2, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == _lib.ERR_DIMENSION_MISMATCH, name
        assert b"negative width" in lib.ngpde_last_error(), name


@pytest.mark.parametrize("aggr", [_lib.AGGR["max"], _lib.AGGR["min"], _lib.AGGR["*"], 7, -1])
def test_fused_propagate_takes_only_sum_and_mean(aggr):
    lib = _lib.load()
    assert lib.ngpde_propagate_emul_forward(None, 8, 1, aggr, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"aggregation" in lib.ngpde_last_error()
    assert lib.ngpde_propagate_emul_backward(None, 8, 1, aggr, None, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"aggregation" in lib.ngpde_last_error()


def test_edge_width_must_be_one_or_the_feature_width():
    lib = _lib.load()
    assert lib.ngpde_propagate_emul_forward(None, 8, 3, 0, None, None, None, None) == _lib.ERR_DIMENSION_MISMATCH
    assert lib.ngpde_gather_forward(None, 5, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_python_api_rejects_an_unknown_aggregation_before_any_device_work():
    g = ng.GNNGraph([1, 1, 2, 3], [2, 3, 1, 1])
    x = np.zeros((2, 3), dtype=np.float32)
    for call in (lambda: ng.propagate(ng.copy_xj, g, "median", xj=x), lambda: ng.aggregate_neighbors(g, "median", np.zeros((2, 4))),
                 lambda: ng.propagate(ng.copy_xj, g, max, xj=x)):
        with pytest.raises(ng.ArgumentError):
            call()
