"""Meshes from points: the Delaunay neighbour graph of 2-D clouds and its triangles, built on the device.

The graphs of the VMH tutorial are Delaunay graphs ([UPSTREAM docs/src/tutorials/VMH.md:53-55]: "Neighbors for each node were
selected by applying Delaunay triangulation to the measurement positions. Two nodes were considered to be neighbors if they lie on
the same edge of at least one triangle.").  The tutorial reads its triangles from a file; `delaunay_graph` gives a new cloud, or one
refined or cut with add_nodes / remove_nodes, the same kind of graph without a host triangulation: no scale parameter, connected,
about 6 neighbours per point at any local density.  Everything runs through the third block of the C ABI (include/ngpde_mesh.h;
csrc/delaunay.hip); there is no CPU fallback.

The rule: i and j are joined iff some closed disk has both on its boundary and no other point of their graph strictly inside.  In
general position that is the Delaunay triangulation's edge set; cocircular points keep every tied diagonal (an integer lattice gives
the 8-neighbour stencil), and tied triangles overlap.  Decisions are made in float64 on the float32 coordinates with a stated
error bound; a decision inside the bound keeps the edge.  Conventions are radius_graph's: points are (2 x n), any real dtype or
stride, on any device (host arrays are moved to the current one); indicators are 1-based graph ids; edges come ordered by point,
the neighbours of a point ascending.  A wrong size raises DimensionMismatch before the library is entered.  There is no gradient to
positions.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .graphs import _device_indicator, _device_points, _graph_from_device_coo
from .layers import _real

__all__ = ["delaunay_graph", "delaunay_triangles"]


def _mismatch(msg):
    return _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, "DimensionMismatch: " + msg)


def _cloud(points, graph_indicator, max_edge_length):
    """shape and value checks on the arrays wherever they live, then the device tensors"""
    t = _real(points if isinstance(points, torch.Tensor) else np.asarray(points), "points")
    if t.dim() != 2 or t.shape[0] != 2:
        raise _mismatch(f"points must be a (2 x n) matrix, got shape {tuple(t.shape)}: the Delaunay graph is built in 2-D")
    if graph_indicator is not None:
        k = graph_indicator.numel() if isinstance(graph_indicator, torch.Tensor) else np.asarray(graph_indicator).size
        if k != t.shape[1]:
            raise _mismatch(f"graph_indicator has {k} entries for {t.shape[1]} points")
    r = math.inf if max_edge_length is None else float(max_edge_length)
    if not r >= 0:
        raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, f"max_edge_length must be >= 0, +inf or None (got {max_edge_length})")
    pts, dev = _device_points(t)
    gi, num_graphs = _device_indicator(graph_indicator, pts.shape[0], dev)
    return pts, dev, gi, num_graphs, r


def delaunay_graph(points, *, graph_indicator=None, max_edge_length=None, dir="in", locality="bfs"):
    """The Delaunay neighbour graph of the (2 x n) points, each graph of `graph_indicator` by itself, as a bidirected GNNGraph with
    its COO lists on the device.  max_edge_length drops every edge longer than it (d2 > r * r under the neighbour search's float32
    rule), which removes the long hull slivers of a sampled cloud; None or +inf keeps everything.  dir="out" swaps s and t;
    locality="spatial" takes the tile schedule from a space-filling curve through the points, as radius_graph does."""
    if dir not in ("in", "out"):
        raise ValueError("dir must be 'in' or 'out'")
    pts, dev, gi, num_graphs, r = _cloud(points, graph_indicator, max_edge_length)
    n = pts.shape[0]
    lib = _lib.load()
    ne = C.c_int64(0)
    args = (n, _lib.ptr(pts), _lib.ptr(gi), num_graphs, 1, r, int(dir == "out"), 0)
    cap = 6 * n + 64                                   # 2 (3n - 6) directed edges without ties: one call fills
    s = torch.empty(cap, dtype=torch.int32, device=dev)
    t = torch.empty(cap, dtype=torch.int32, device=dev)
    status = lib.ngpde_delaunay_graph(*args, cap, _lib.ptr(s), _lib.ptr(t), C.byref(ne), _lib.current_stream())
    if status != _lib.OK and ne.value > cap:           # ties: the count is known now
        cap = int(ne.value)
        s = torch.empty(cap, dtype=torch.int32, device=dev)
        t = torch.empty(cap, dtype=torch.int32, device=dev)
        status = lib.ngpde_delaunay_graph(*args, cap, _lib.ptr(s), _lib.ptr(t), C.byref(ne), _lib.current_stream())
    _lib.check(status)
    m = int(ne.value)
    return _graph_from_device_coo(s[:m].clone(), t[:m].clone(), n, num_graphs, dev, pts, gi, locality)


def delaunay_triangles(points, *, graph_indicator=None, max_edge_length=None):
    """The triangles of the Delaunay graph: an int32 [T, 3] tensor on the device, 0-based, every triangle once as (i, j, k)
    counter-clockwise with i its smallest index, sorted lexicographically.  A triangle with an edge longer than max_edge_length is
    dropped.  Tied (cocircular) triangles overlap."""
    pts, dev, gi, num_graphs, r = _cloud(points, graph_indicator, max_edge_length)
    n = pts.shape[0]
    lib = _lib.load()
    nt = C.c_int64(0)
    args = (n, _lib.ptr(pts), _lib.ptr(gi), num_graphs, 1, r, 0)
    cap = 2 * n + 64
    tri = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    status = lib.ngpde_delaunay_triangles(*args, cap, _lib.ptr(tri), C.byref(nt), _lib.current_stream())
    if status != _lib.OK and nt.value > cap:
        cap = int(nt.value)
        tri = torch.empty((cap, 3), dtype=torch.int32, device=dev)
        status = lib.ngpde_delaunay_triangles(*args, cap, _lib.ptr(tri), C.byref(nt), _lib.current_stream())
    _lib.check(status)
    return tri[:int(nt.value)].clone()
