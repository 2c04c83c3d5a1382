"""Relating two point sets: the k nearest / all within r DATA points of every QUERY point, and k-nearest-neighbour interpolation of
node features from one cloud onto another -- comparing a learned solution with data given on other points, putting a field on a
regular grid, initialising a fine cloud from a coarse solve, carrying features across add_nodes / remove_nodes.

[UPSTREAM NearestNeighbors.jl: knn(tree, queries, k), inrange(tree, queries, r) over the trees GNNGraphs.knn_graph / radius_graph
are built on; torch_geometric's knn_interpolate for the interpolation.]  Everything runs on the device through the second block
of the C ABI (include/ngpde_interp.h; csrc/neighbors.hip, csrc/interp.hip); there is no CPU fallback and no M x N distance matrix.

Conventions: points and queries are (dim x n) as radius_graph takes them, dim <= 3; indicators are 1-based graph ids as in
GNNGraphs, and a query is searched among the points of its own graph only; positions (idx, neighbours) are 0-based.  The decision
rule is the neighbour search's float rule (sum of float squares in coordinate order, ties by index), so the lists are the
brute-force lists bit for bit.  Real arrays follow the one rule of layers.rows_of: any real dtype, stride or offset in, float32
contiguous to the kernels; host arrays are moved to the current device as radius_graph moves its points.  A wrong size raises
DimensionMismatch before the library is entered.  There is no gradient to positions: upstream's knn gives none either.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .layers import _real, rows_of
from .queries import AdjacencyList

__all__ = ["knn", "inrange", "KNNInterpolator", "knn_interpolate"]


def _mismatch(msg):
    return _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, "DimensionMismatch: " + msg)


def _matrix(a, what):
    """the (dim x n) array as a tensor wherever it lives: shape checks come before the device is asked for"""
    t = _real(a if isinstance(a, torch.Tensor) else np.asarray(a), what)
    if t.dim() == 1:
        t = t.reshape(1, -1)
    if t.dim() != 2:
        raise _mismatch(f"{what} must be a (dim x n) matrix, got shape {tuple(t.shape)}")
    return t


def _indicator(gi, n, what, of):
    if gi is None:
        return None
    g = gi if isinstance(gi, torch.Tensor) else torch.as_tensor(np.asarray(gi))
    g = g.reshape(-1)
    if g.numel() != n:
        raise _mismatch(f"{what} has {g.numel()} entries for {n} {of}")
    return g


def _device():
    if not torch.cuda.is_available():
        raise _lib.NgpdeError(_lib.ERR_HIP, "no HIP device: the two-set search and the interpolation run on the GPU "
                                            "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


class _Sets:
    """the checked arguments of one two-set call on the device: pts [n][dim], qs [m][dim], the indicators or None, n_graphs"""

    def __init__(self, points, queries, graph_indicator, query_graph_indicator):
        p, q = _matrix(points, "points"), _matrix(queries, "queries")
        if p.shape[0] != q.shape[0]:
            raise _mismatch(f"points have {p.shape[0]} coordinates, queries have {q.shape[0]}")
        if not 1 <= p.shape[0] <= 3:
            raise _mismatch(f"the neighbour search takes 1, 2 or 3 coordinates, points have {p.shape[0]}")
        self.dim, self.n, self.m = int(p.shape[0]), int(p.shape[1]), int(q.shape[1])
        gp = _indicator(graph_indicator, self.n, "graph_indicator", "points")
        gq = _indicator(query_graph_indicator, self.m, "query_graph_indicator", "queries")
        self.dev = dev = _device()
        self.pts, self.qs = rows_of(p.to(dev)), rows_of(q.to(dev))
        self.gp = self.gq = None
        self.n_graphs = 1
        if gp is not None or gq is not None:      # a side without an indicator lies in graph 1
            ones = lambda k: torch.ones(k, dtype=torch.int32, device=dev)
            self.gp = ones(self.n) if gp is None else gp.to(dev, torch.int32).contiguous()
            self.gq = ones(self.m) if gq is None else gq.to(dev, torch.int32).contiguous()
            tops = [int(g.max().item()) for g in (self.gp, self.gq) if g.numel()]
            self.n_graphs = max(tops + [1])       # 1-based ids as in GNNGraphs: the number of graphs is the largest id

    def head(self):
        return (self.n, self.m, self.dim, _lib.ptr(self.pts), _lib.ptr(self.qs))

    def tail(self):
        return (_lib.ptr(self.gp), _lib.ptr(self.gq), self.n_graphs, 1, 0)


def _count(k):
    if isinstance(k, bool) or int(k) != k or int(k) < 0:
        raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, f"k must be a non-negative integer, got {k!r}")
    return int(k)


def _knn_rows(points, queries, k, graph_indicator, query_graph_indicator):
    k = _count(k)
    a = _Sets(points, queries, graph_indicator, query_graph_indicator)
    idx = torch.empty((a.m, k), dtype=torch.int32, device=a.dev)
    d2 = torch.empty((a.m, k), dtype=torch.float32, device=a.dev)
    _lib.check(_lib.load().ngpde_knn_query(*a.head(), k, *a.tail(), _lib.ptr(idx), _lib.ptr(d2), _lib.current_stream()))
    return a, idx, d2


def knn(points, queries, k, *, graph_indicator=None, query_graph_indicator=None):
    """[UPSTREAM NearestNeighbors.knn(tree, queries, k, sortres = true)] the k nearest points of every query: (idx, d2), both
    (k x M), column q holding the 0-based positions (int32) and squared float distances of query q's neighbours, nearest first,
    equal distances by position.  A query whose graph holds fewer than k points is an ArgumentError that names the graph."""
    _, idx, d2 = _knn_rows(points, queries, k, graph_indicator, query_graph_indicator)
    return idx.T, d2.T


def inrange(points, queries, r, *, graph_indicator=None, query_graph_indicator=None):
    """[UPSTREAM NearestNeighbors.inrange(tree, queries, r)] the points within distance r (<=, decided as d2 <= r*r in float) of
    every query: an AdjacencyList with one row per query, `neighbors` the 0-based positions ascending, `eid` None."""
    a = _Sets(points, queries, graph_indicator, query_graph_indicator)
    lib = _lib.load()
    found = C.c_int64(0)
    _lib.check(lib.ngpde_radius_query(*a.head(), float(r), *a.tail(), 0, None, None, C.byref(found), _lib.current_stream()))
    total = int(found.value)
    ptr = torch.zeros(a.m + 1, dtype=torch.int32, device=a.dev)
    nbr = torch.empty(max(total, 1), dtype=torch.int32, device=a.dev)
    _lib.check(lib.ngpde_radius_query(*a.head(), float(r), *a.tail(), total, _lib.ptr(ptr), _lib.ptr(nbr), C.byref(found),
                                      _lib.current_stream()))
    return AdjacencyList(ptr, nbr[:total], None)


class _Interpolate(torch.autograd.Function):
    """y = A x over the rows [N][D] -> [M][D]; the pullback is A' ybar.  Two launches, nothing allocated by the library."""

    @staticmethod
    def forward(ctx, itp, xr):
        ctx.itp = itp
        y = torch.empty((itp.num_queries, xr.shape[1]), dtype=torch.float32, device=xr.device)
        _lib.check(_lib.load().ngpde_knn_interp_forward(itp.num_points, itp.num_queries, itp.k, xr.shape[1], _lib.ptr(itp._idx),
                                                        _lib.ptr(itp._w), _lib.ptr(xr), _lib.ptr(y), _lib.current_stream()))
        return y

    @staticmethod
    def backward(ctx, ybar):
        itp = ctx.itp
        ptr, slot = itp.transpose()
        ybar = ybar.to(torch.float32).contiguous()
        xbar = torch.empty((itp.num_points, ybar.shape[1]), dtype=torch.float32, device=ybar.device)
        _lib.check(_lib.load().ngpde_knn_interp_backward(itp.num_points, itp.num_queries, itp.k, ybar.shape[1], _lib.ptr(ptr),
                                                         _lib.ptr(slot), _lib.ptr(itp._w), _lib.ptr(ybar), _lib.ptr(xbar),
                                                         _lib.current_stream()))
        return None, xbar


class KNNInterpolator:
    """Shepard interpolation from `points` onto `queries` over the k nearest points of every query ([UPSTREAM torch_geometric's
    knn_interpolate], normalised by the nearest distance instead of clamped at 1e-16: with c_j = max(d2_j, FLT_MIN) the weights are
    w_j = c_0 / c_j, all 1 where c_0 is inf, and y = sum_j w_j x[idx_j] / sum_j w_j -- scale-free, nothing over- or underflows, and
    coincident points share the value equally).  The search runs once, here; `idx`, `d2` and `weights` (the normalised w_j / W)
    are (k x M) and kept, the by-point transpose the pullback walks is built on first need (or by `transpose()`, e.g. ahead of a
    HIP-graph capture).  `itp(x)` maps (D x N) to (D x M) and is differentiable in x; positions get no gradient."""

    def __init__(self, points, queries, k=3, *, graph_indicator=None, query_graph_indicator=None):
        a, self._idx, self._d2 = _knn_rows(points, queries, k, graph_indicator, query_graph_indicator)
        self.num_points, self.num_queries, self.k, self.device = a.n, a.m, int(self._idx.shape[1]), a.dev
        self._w = torch.empty_like(self._d2)
        _lib.check(_lib.load().ngpde_knn_interp_weights(a.m, self.k, _lib.ptr(self._d2), _lib.ptr(self._w), _lib.current_stream()))
        self.idx, self.d2, self.weights = self._idx.T, self._d2.T, self._w.T
        self._rows = None

    def transpose(self):
        """(ptr, slot): slot[ptr[i] : ptr[i + 1]] are the positions q * k + j that name point i, ascending"""
        if self._rows is None:
            lib = _lib.load()
            n, m, k = self.num_points, self.num_queries, self.k
            ptr = torch.empty(n + 1, dtype=torch.int32, device=self.device)
            slot = torch.empty(m * k, dtype=torch.int32, device=self.device)
            nbytes = int(lib.ngpde_knn_interp_transpose_workspace_bytes(n, m, k))
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
            _lib.check(lib.ngpde_knn_interp_transpose(n, m, k, _lib.ptr(self._idx), _lib.ptr(ptr), _lib.ptr(slot), _lib.ptr(ws), nbytes,
                                                      _lib.current_stream()))
            self._rows = (ptr, slot)
        return self._rows

    def __call__(self, x):
        x = _real(x if isinstance(x, torch.Tensor) else np.asarray(x), "x")
        if x.dim() != 2 or x.shape[1] != self.num_points:
            raise _mismatch(f"x must be (D x {self.num_points}), one column per point, got shape {tuple(x.shape)}")
        return _Interpolate.apply(self, rows_of(x.to(self.device))).T

    def matrix_rows(self):
        """(idx, weights), both (k x M): row q of the interpolation matrix has the entries weights[:, q] in the columns idx[:, q]"""
        return self.idx, self.weights

    def __repr__(self):
        return f"KNNInterpolator({self.num_points} points -> {self.num_queries} queries, k = {self.k})"


def knn_interpolate(x, points, queries, k=3, **kw):
    """the one-shot form: KNNInterpolator(points, queries, k, **kw)(x); x is (D x N), the result (D x M)"""
    x = _real(x if isinstance(x, torch.Tensor) else np.asarray(x), "x")
    n = _matrix(points, "points").shape[1]
    if x.dim() != 2 or x.shape[1] != n:
        raise _mismatch(f"x must be (D x {n}), one column per point, got shape {tuple(x.shape)}")
    return KNNInterpolator(points, queries, k, **kw)(x)
