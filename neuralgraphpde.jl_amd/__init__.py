"""neuralgraphpde.jl_amd -- MI355X-native message-passing hot path of NeuralGraphPDE.jl behind the
reference's Lux explicit-layer API.  Import it as `ngpde_amd` (the directory name contains a dot,
so the repo-root shim ngpde_amd.py loads it under that name).

Everything that computes goes through libngpde_hip.so (include/ngpde.h); there is no CPU fallback.
"""
from . import _lib
from ._lib import ArgumentError, DimensionMismatch, NgpdeError
from .graphs import EMPTYGRAPH, GNNGraph, batch, knn_graph, radius_graph, rand_graph
from .utils import drop, updategraph, wrapgraph
from .layers import (AbstractExplicitLayer, AbstractGNNContainerLayer, AbstractGNNLayer, Chain, Dense,
                     GCNConv, apply, glorot_normal, glorot_uniform, setup, to_device, zeros32)
from .node import NeuralODE
from .layers_mp import ExplicitEdgeConv, GATConv, GNOConv, MPPDEConv, SpectralConv, VMHConv
from .msgpass import (aggregate_neighbors, apply_edges, copy_xi, copy_xj, e_mul_xj, propagate, softmax_edge_neighbors, w_mul_xj,
                      xi_dot_xj)
from .readout import (broadcast_edges, broadcast_nodes, graph_indicator, reduce_edges, reduce_nodes, softmax_edges, softmax_nodes)
from .graphops import (add_self_loops, degree, getgraph, has_multi_edges, has_self_loops, induced_subgraph, is_bidirected,
                       remove_multi_edges, remove_self_loops, to_bidirected, unbatch)
from .sampling import rand_edge_split, sample_neighbors
from .editing import (add_edges, add_nodes, get_edge_weight, negative_sample, remove_edges, remove_nodes, set_edge_weight,
                      to_unidirected)
from .matrices import (GraphMatrix, adjacency_matrix, has_isolated_nodes, khop_adj, laplacian_lambda_max, laplacian_matrix,
                       normalized_laplacian, scaled_laplacian)
from .queries import (AdjacencyList, adjacency_list, has_edge, inneighbors, intersect, neighbors, outneighbors, random_walk_pe)
from .linsolve import CGInfo, cg_solve
from .traversal import (Components, ShortestPaths, connected_components, hop_distance, is_connected, neighborhood, shortest_paths,
                        split_components)
from . import dist, optim, synth, interp, mesh, coarsen


def release_cached_memory():
    """device memory the library keeps parked for re-use (the tapes of destroyed NeuralODE(VMHConv) plans) back to the device; bytes released
    (the analogue of CUDA.reclaim() / torch.cuda.empty_cache() for the library's own allocations)"""
    _lib.flush_destroy()
    return int(_lib.load().ngpde_release_cached_memory())

__all__ = [
    "AbstractExplicitLayer", "AbstractGNNLayer", "AbstractGNNContainerLayer", "GCNConv", "Dense", "Chain", "NeuralODE",
    "ExplicitEdgeConv", "VMHConv", "MPPDEConv", "GNOConv", "SpectralConv", "GATConv",
    "setup", "apply", "to_device", "updategraph", "wrapgraph", "drop", "GNNGraph", "EMPTYGRAPH", "rand_graph",
    "batch", "radius_graph", "knn_graph", "glorot_uniform", "glorot_normal", "zeros32", "NgpdeError", "DimensionMismatch", "ArgumentError",
    "propagate", "apply_edges", "aggregate_neighbors", "softmax_edge_neighbors", "copy_xj", "copy_xi", "xi_dot_xj", "e_mul_xj", "w_mul_xj",
    "reduce_nodes", "reduce_edges", "softmax_nodes", "softmax_edges", "broadcast_nodes", "broadcast_edges", "graph_indicator",
    "degree", "has_self_loops", "has_multi_edges", "is_bidirected", "add_self_loops", "remove_self_loops", "remove_multi_edges",
    "to_bidirected", "induced_subgraph", "getgraph", "unbatch", "sample_neighbors", "rand_edge_split",
    "add_nodes", "add_edges", "remove_edges", "remove_nodes", "to_unidirected", "set_edge_weight", "get_edge_weight", "negative_sample",
    "GraphMatrix", "adjacency_matrix", "laplacian_matrix", "normalized_laplacian", "scaled_laplacian", "laplacian_lambda_max", "khop_adj",
    "has_isolated_nodes", "cg_solve", "CGInfo",
    "AdjacencyList", "adjacency_list", "has_edge", "neighbors", "inneighbors", "outneighbors", "intersect", "random_walk_pe",
    "Components", "connected_components", "is_connected", "split_components", "hop_distance", "neighborhood",
    "ShortestPaths", "shortest_paths",
]
