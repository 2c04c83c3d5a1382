"""Choosing the coarse cloud: farthest-point sampling, grid clusters and pooling over clusters -- the levels of a multi-level graph
kernel network, a coarse-to-fine solve, a pooled read-out between message-passing layers -- without a round trip through host numpy.

[UPSTREAM torch_geometric: fps, voxel_grid, avg_pool / max_pool / avg_pool_x; the "unpool" they pair with is
interp.knn_interpolate.]  Everything runs on the device through the fourth block of the C ABI (include/ngpde_coarsen.h;
csrc/coarsen.hip, the rules in csrc/coarsen_rule.h); there is no CPU fallback.

Conventions are those of interp.py: points are (dim x n), dim 1 to 3; any real dtype, stride or offset comes in and the kernels get
float32 contiguous; host arrays are moved to the current device; `graph_indicator` holds 1-based graph ids; positions out are
0-based int32; a wrong shape is a DimensionMismatch raised before the library is entered; no gradient flows to positions.  Here the
indicator must be NON-DECREASING, which every batch() gives: anything else is an ArgumentError that names the first position where
it decreases (found in the same read-back that fetches the graph sizes).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .interp import _device, _indicator, _matrix, _mismatch
from .layers import _real, rows_of
from .sampling import _seed_of

__all__ = ["fps", "grid_cluster", "Clusters", "pool", "pool_positions", "pool_graph"]

TILE_MAX_POINTS = 16384      # NGPDE_FPS_TILE_MAX_POINTS
TILE_THREADS = 1024          # NGPDE_FPS_TILE_THREADS
_PATHS = {"auto": 0, "tile": 1, "round": 2}
_AGGRS = {k: _lib.AGGR[k] for k in ("+", "sum", "add", "mean", "max", "min")}


def _arg_error(msg):
    return _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, msg)


def _points(points):
    p = _matrix(points, "points")
    if not 1 <= p.shape[0] <= 3:
        raise _mismatch(f"points must have 1, 2 or 3 coordinates, got {p.shape[0]}")
    return p


def _graph_ptr(gi, n, what="graph_indicator"):
    """the bounds (host int64 [G + 1]) of the graphs of a non-decreasing 1-based indicator; a device indicator costs one read-back"""
    if gi is None:
        return np.array([0, n], dtype=np.int64)
    if n == 0:
        return np.array([0, 0], dtype=np.int64)
    if gi.is_cuda:
        g = gi.to(torch.int64)
        vals, counts = torch.unique_consecutive(g, return_counts=True)
        drop = g[1:] < g[:-1]
        first = torch.where(drop.any(), drop.to(torch.int8).argmax(), torch.full((), -1, device=g.device))
        packed = torch.cat([first.reshape(1), vals, counts]).cpu().numpy()         # the one read-back: sizes and monotonicity
        first, vals, counts = int(packed[0]), packed[1:1 + vals.numel()], packed[1 + vals.numel():]
    else:
        a = gi.to(torch.int64).numpy()
        drop = np.flatnonzero(a[1:] < a[:-1])
        first = int(drop[0]) if drop.size else -1
        starts = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
        vals, counts = a[starts], np.diff(np.append(starts, a.size))
    if first >= 0:
        raise _arg_error(f"{what} must be non-decreasing (as batch() gives it): it decreases at position {first + 1}")
    if vals[0] < 1:
        raise _arg_error(f"{what} holds the id {int(vals[0])}: graph ids are 1-based")
    sizes = np.zeros(int(vals[-1]), dtype=np.int64)
    sizes[vals - 1] = counts
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


def _sample_counts(num, ratio, ptr):
    sizes = np.diff(ptr)
    G = sizes.size
    if (num is None) == (ratio is None):
        raise _arg_error("fps: exactly one of num and ratio must be given")
    if ratio is not None:
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0 < float(ratio) <= 1:
            raise _arg_error(f"fps: ratio must lie in (0, 1], got {ratio!r}")
        ks = np.array([math.ceil(float(ratio) * int(n)) for n in sizes], dtype=np.int64)
    else:
        a = np.asarray(num.cpu() if isinstance(num, torch.Tensor) else num)
        if a.dtype == bool or not np.issubdtype(a.dtype, np.integer) or a.ndim > 1 or (a.ndim == 1 and a.size != G):
            raise _arg_error(f"fps: num must be an integer or one integer per graph ({G}), got {num!r}")
        ks = np.broadcast_to(a.astype(np.int64), (G,)).copy()
        if (ks < 0).any():
            raise _arg_error(f"fps: num must be >= 0, got {num!r}")
    over = np.flatnonzero(ks > sizes)
    if over.size:
        g = int(over[0])
        raise _arg_error(f"fps: graph {g + 1} has {int(sizes[g])} points, {int(ks[g])} samples asked for")
    return ks


def _starts(start, random_start, seed, ptr):
    """the start position of every graph (host int32 [G]) or None for every graph's first point"""
    G = ptr.size - 1
    if start is not None and random_start:
        raise _arg_error("fps: start and random_start exclude each other")
    if random_start:
        gen = torch.Generator()
        gen.manual_seed(_seed_of(seed, "fps"))
        return np.array([int(ptr[g]) + (int(torch.randint(int(ptr[g + 1] - ptr[g]), (1,), generator=gen).item()) if ptr[g + 1] > ptr[g] else 0)
                         for g in range(G)], dtype=np.int32)
    if start is None:
        return None
    s = np.asarray(start.cpu() if isinstance(start, torch.Tensor) else start).reshape(-1)
    if s.size != G:
        raise _mismatch(f"start has {s.size} entries for {G} graphs")
    if not np.array_equal(s, np.floor(s)):
        raise _arg_error("fps: start must hold integer positions")
    s = s.astype(np.int64)
    for g in range(G):
        if ptr[g + 1] > ptr[g] and not ptr[g] <= s[g] < ptr[g + 1]:
            raise _arg_error(f"fps: start {int(s[g])} lies outside graph {g + 1}, whose points are {int(ptr[g])}:{int(ptr[g + 1]) - 1}")
    return s.astype(np.int32)


def _run_fps(pts, ptr, ks, starts, path="auto"):
    """the C plan and the call: pts [n][dim] on the device; (idx, d2, info) with info = ngpde_fps_plan_info's six numbers"""
    lib = _lib.load()
    dev = pts.device
    G = ptr.size - 1
    gp = np.ascontiguousarray(ptr, dtype=np.int64)
    sp = np.concatenate(([0], np.cumsum(ks))).astype(np.int64)
    plan = C.c_void_p()
    _lib.check(lib.ngpde_fps_plan_create(G, _lib.ptr(gp), _lib.ptr(sp), int(pts.shape[1]), _PATHS[path], _lib.current_stream(), C.byref(plan)))
    try:
        info = (C.c_int64 * 6)()
        _lib.check(lib.ngpde_fps_plan_info(plan, info))
        K = int(sp[-1])
        idx = torch.empty(K, dtype=torch.int32, device=dev)
        d2 = torch.empty(K, dtype=torch.float32, device=dev)
        nbytes = int(lib.ngpde_fps_workspace_bytes(plan))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        st = None if starts is None else torch.as_tensor(starts, dtype=torch.int32).to(dev)
        _lib.check(lib.ngpde_fps(plan, _lib.ptr(pts), _lib.ptr(st), 0, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(ws), nbytes, _lib.current_stream()))
    finally:
        _lib.destroy_later("ngpde_fps_plan_destroy", plan)
    return idx, d2, list(info)


def fps(points, *, num=None, ratio=None, graph_indicator=None, start=None, random_start=False, seed=None, return_d2=False):
    """[UPSTREAM torch_geometric.nn.fps] farthest-point sampling of every graph: `idx`, int32 [K], the 0-based positions of the samples,
    graphs concatenated, each graph's samples in SELECTION ORDER; with return_d2=True `(idx, d2)`, d2[r] being the squared float
    distance of sample r to the samples before it (inf for a graph's first; a graph's last bounds the covering radius of its
    sample).  The graph of a sample is graph_indicator[idx].

    The rule (include/ngpde_coarsen.h) is a pure function of the arguments: round 0 takes the start point, every later round the
    point farthest from the chosen set in the neighbour search's float distance, equal distances going to the smallest index.
    Selection order makes results NESTED: fps(num=a) is a prefix of fps(num=b) for a < b at the same start, so one call yields
    every level of a hierarchy.

    num: an int, the same for every graph, or one per graph; ratio: k_g = math.ceil(ratio * n_g), 0 < ratio <= 1; exactly one of the
    two.  More samples than a graph has points is an ArgumentError naming the graph; 0 samples and empty graphs are fine.
    start: one 0-based global position per graph (None: each graph's first point); a start outside its graph is an ArgumentError.
    random_start=True draws the starts graph by graph, in order, as lo_g + torch.randint(n_g, (1,), generator=gen) from a CPU
    torch.Generator seeded with `seed` (seed=None takes a seed from torch's CPU generator, as sample_neighbors does).
    The DEFAULT IS DETERMINISTIC (random_start=False): a deliberate difference from torch_geometric's random_start=True."""
    p = _points(points)
    n = int(p.shape[1])
    gi = _indicator(graph_indicator, n, "graph_indicator", "points")
    if gi is not None:
        gi = _real(gi, "graph_indicator")
    ptr = _graph_ptr(gi, n)
    ks = _sample_counts(num, ratio, ptr)
    starts = _starts(start, random_start, seed, ptr)
    dev = _device()
    idx, d2, _ = _run_fps(rows_of(p.to(dev)), ptr, ks, starts)
    return (idx, d2) if return_d2 else idx


# ---- clusters -------------------------------------------------------------------------------------------------------------------
def _rows_of_labels(labels, count):
    """(ptr, order) of labels [N] with values 0 : count-1: the structure ngpde_knn_interp_transpose builds for k = 1"""
    lib = _lib.load()
    n, dev = int(labels.numel()), labels.device
    ptr = torch.empty(count + 1, dtype=torch.int32, device=dev)
    order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    nbytes = int(lib.ngpde_knn_interp_transpose_workspace_bytes(count, n, 1))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.ngpde_knn_interp_transpose(count, n, 1, _lib.ptr(labels), _lib.ptr(ptr), _lib.ptr(order), _lib.ptr(ws), nbytes,
                                              _lib.current_stream()))
    return ptr, order[:n]


class Clusters:
    """A partition of N points into `count` clusters, all on the device: `labels` int32 [N] (0-based), `ptr` int32 [count + 1] and
    `order` int32 [N] (the members of cluster c are order[ptr[c] : ptr[c + 1]], ascending by node), `sizes` int32 [count],
    `graph_indicator` int32 [count] (1-based; non-decreasing, so the coarse set is again a batch) and `num_graphs`."""

    def __init__(self, labels, count, ptr, order, graph_indicator, num_graphs):
        self.labels, self.count, self.ptr, self.order = labels, int(count), ptr, order
        self.sizes = ptr[1:] - ptr[:-1]
        self.graph_indicator, self.num_graphs = graph_indicator, int(num_graphs)
        self.num_points, self.device = int(labels.numel()), labels.device

    @classmethod
    def from_labels(cls, labels, graph_indicator=None):
        """wrap labels of one's own (a k-means, say): int [N] with every value of 0 : max occurring; with a `graph_indicator` (1-based,
        [N]) every cluster must lie in one graph and the clusters' graphs must be non-decreasing"""
        lab = _real(labels if isinstance(labels, torch.Tensor) else np.asarray(labels), "labels").reshape(-1)
        n = int(lab.numel())
        gi = _indicator(graph_indicator, n, "graph_indicator", "points")
        dev = _device()
        lab = lab.to(dev).to(torch.int32).contiguous()
        if n == 0:
            e = torch.zeros(0, dtype=torch.int32, device=dev)
            return cls(e, 0, torch.zeros(1, dtype=torch.int32, device=dev), e, e, 1)
        lo, hi = (int(v) for v in torch.stack([lab.min(), lab.max()]).cpu())
        if lo < 0:
            raise _arg_error(f"Clusters.from_labels: labels are 0-based, got {lo}")
        count = hi + 1
        ptr, order = _rows_of_labels(lab, count)
        sizes = ptr[1:] - ptr[:-1]
        first = order[ptr[:-1].long().clamp(max=n - 1)].long()
        g = torch.ones(n, dtype=torch.int32, device=dev) if gi is None else _real(gi, "graph_indicator").to(dev).to(torch.int32)
        cg = g[first]
        bad = torch.stack([(sizes == 0).any(), (cg[lab.long()] != g).any(), (cg[1:] < cg[:-1]).any()])
        flags = torch.cat([bad.to(torch.int32), g.max().reshape(1)]).cpu().tolist()       # one read-back
        if flags[0]:
            raise _arg_error("Clusters.from_labels: every label of 0 : max must occur (an empty cluster has no graph)")
        if flags[1]:
            raise _arg_error("Clusters.from_labels: a cluster holds points of more than one graph")
        if flags[2]:
            raise _arg_error("Clusters.from_labels: the clusters' graphs must be non-decreasing in the label")
        return cls(lab, count, ptr, order, cg.contiguous(), int(flags[3]))

    def unpool(self, xc):
        """(D x count) -> (D x N): xc[:, labels], a gather whose pullback is the "+" pool"""
        xc = _real(xc if isinstance(xc, torch.Tensor) else np.asarray(xc), "xc")
        if xc.dim() != 2 or xc.shape[1] != self.count:
            raise _mismatch(f"xc must be (D x {self.count}), one column per cluster, got shape {tuple(xc.shape)}")
        return _Unpool.apply(self, rows_of(xc.to(self.device))).T

    def __repr__(self):
        return f"Clusters({self.num_points} points -> {self.count} clusters, {self.num_graphs} graphs)"


def _per_coordinate(v, dim, what):
    a = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, dim)
    if a.size != dim:
        raise _mismatch(f"{what} has {a.size} entries for {dim} coordinates")
    return a.astype(np.float32)


def grid_cluster(points, size, *, graph_indicator=None, origin=None):
    """[UPSTREAM torch_geometric.nn.voxel_grid] two points share a cluster iff they share graph and cell, the cell of a coordinate being
    (int32) floorf((p - o) / size) in float.  size: a scalar or one value per coordinate, finite and > 0.  o: by default the minimum of
    the graph's OWN points per coordinate, so a graph clusters the same way alone or inside a batch; with origin=(dim,) that point
    for all graphs (a point below it is refused by name, as is a non-finite coordinate).  Clusters are numbered by ascending
    (graph, c_z, c_y, c_x), x fastest.  A cell size too small for the cloud's extent (a key beyond 63 bits) is refused by name."""
    p = _points(points)
    dim, n = int(p.shape[0]), int(p.shape[1])
    gi = _indicator(graph_indicator, n, "graph_indicator", "points")
    h = _per_coordinate(size, dim, "size")
    if not (np.isfinite(h).all() and (h > 0).all()):
        raise _arg_error(f"grid_cluster: size must be finite and > 0, got {size!r}")
    o = None if origin is None else _per_coordinate(origin, dim, "origin")
    if o is not None and not np.isfinite(o).all():
        raise _arg_error(f"grid_cluster: origin must be finite, got {origin!r}")
    ptr_g = _graph_ptr(None if gi is None else _real(gi, "graph_indicator"), n)
    dev = _device()
    pts = rows_of(p.to(dev))
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    labels, ptr, order, cg = i32(n), i32(n + 1), i32(n), i32(n)
    count = C.c_int64(0)
    G = ptr_g.size - 1
    _lib.check(_lib.load().ngpde_grid_cluster(n, dim, _lib.ptr(pts), G, _lib.ptr(ptr_g), _lib.ptr(h), _lib.ptr(o), _lib.ptr(labels), _lib.ptr(ptr),
                                              _lib.ptr(order), _lib.ptr(cg), C.byref(count), _lib.current_stream()))
    c = int(count.value)
    return Clusters(labels, c, ptr[:c + 1], order, cg[:c], G)


# ---- pooling --------------------------------------------------------------------------------------------------------------------
def _pool_backward(cl, aggr, x, out, dout):
    n, d = cl.num_points, int(dout.shape[1])
    dx = torch.empty((n, d), dtype=torch.float32, device=dout.device)
    _lib.check(_lib.load().ngpde_cluster_pool_backward(n, cl.count, d, aggr, _lib.ptr(cl.labels), _lib.ptr(cl.ptr), _lib.ptr(x), _lib.ptr(out),
                                                       _lib.ptr(dout), _lib.ptr(dx), _lib.current_stream()))
    return dx


def _pool_forward(cl, aggr, x):
    d = int(x.shape[1])
    out = torch.empty((cl.count, d), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ngpde_cluster_pool_forward(cl.num_points, cl.count, d, aggr, _lib.ptr(cl.ptr), _lib.ptr(cl.order), _lib.ptr(x),
                                                      _lib.ptr(out), _lib.current_stream()))
    return out


class _Pool(torch.autograd.Function):
    """x [N][D] -> [C][D] over the clusters' rows; the pullback is one gather launch"""

    @staticmethod
    def forward(ctx, cl, aggr, x):
        x = x.contiguous()
        out = _pool_forward(cl, aggr, x)
        ctx.cl, ctx.aggr = cl, aggr
        if aggr in (_lib.AGGR["max"], _lib.AGGR["min"]):
            ctx.save_for_backward(x, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out = ctx.saved_tensors if ctx.saved_tensors else (None, None)
        return None, None, _pool_backward(ctx.cl, ctx.aggr, x, out, dout.to(torch.float32).contiguous())


class _Unpool(torch.autograd.Function):
    """xc [C][D] -> [N][D]: the gather is the "+" pool's pullback, and its own pullback the "+" pool"""

    @staticmethod
    def forward(ctx, cl, xc):
        ctx.cl = cl
        return _pool_backward(cl, _lib.AGGR["+"], None, None, xc.contiguous())

    @staticmethod
    def backward(ctx, dx):
        return None, _pool_forward(ctx.cl, _lib.AGGR["+"], dx.to(torch.float32).contiguous())


def pool(clusters, x, aggr="mean"):
    """[UPSTREAM torch_geometric's avg_pool_x / max_pool_x] x (D x N) -> (D x count): every cluster's members combined with aggr, "+",
    "mean", "max" or "min"; float32, differentiable in x (max / min send the gradient to every tied entry), atomic-free and the same
    bits on every run (the order contract is in include/ngpde_coarsen.h)."""
    code = _AGGRS.get(aggr) if isinstance(aggr, str) else None
    if code is None:
        raise _arg_error(f"unsupported aggregation {aggr!r}; clusters are pooled with '+', 'mean', 'max' or 'min'")
    x = _real(x if isinstance(x, torch.Tensor) else np.asarray(x), "x")
    if x.dim() != 2 or x.shape[1] != clusters.num_points or x.shape[0] < 1:
        raise _mismatch(f"x must be (D x {clusters.num_points}), one column per point and D >= 1, got shape {tuple(x.shape)}")
    return _Pool.apply(clusters, code, rows_of(x.to(clusters.device))).T


def pool_positions(clusters, points):
    """the clusters' centroids, (dim x count): pool(clusters, points, "mean")"""
    return pool(clusters, _matrix(points, "points"), "mean")


def pool_graph(g, clusters, aggr="+"):
    """[UPSTREAM torch_geometric's pool_edge] the coarse GNNGraph: every edge (s, t) becomes (label_s, label_t), loops are dropped and
    duplicate edges merged as remove_multi_edges(g, aggr) does -- edges come out by source then target, `edge_weight` and float edge
    features are combined by aggr with their gradients.  The result carries clusters.graph_indicator; node features are not carried
    (pool them with `pool`)."""
    from . import graphops
    if g.num_nodes != clusters.num_points:
        raise _mismatch(f"the graph has {g.num_nodes} nodes, the clusters cover {clusters.num_points} points")
    graphops._aggr_code(aggr)
    dev = clusters.device
    s, t = graphops._coo(g, dev)
    lab = clusters.labels
    cs, ct = lab[s.long()].contiguous(), lab[t.long()].contiguous()
    indicator = (clusters.graph_indicator - 1).cpu().numpy() if clusters.num_graphs > 1 else None
    coarse = graphops._new_graph(cs, ct, clusters.count, dev, num_graphs=clusters.num_graphs, indicator=indicator, ndata=None,
                                 edata=dict(g.edata), gdata=dict(g.gdata), edge_weight=g.edge_weight)
    return graphops.remove_multi_edges(graphops.remove_self_loops(coarse), aggr)
