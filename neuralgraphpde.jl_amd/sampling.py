"""Random parts of a graph: `sample_neighbors` and `rand_edge_split` of the GNNGraphs re-export (src/NeuralGraphPDE.jl:4 of the
reference) -- the fresh sub-sampled neighbourhoods a graph kernel network trains on every epoch, a cap on a hub's row, an edge hold-out:

    gs = sample_neighbors(g, None, 8, seed=epoch)            # at most 8 inbound edges per node, a uniform subset of each row
    st = updategraph(st, gs)
    train, held = rand_edge_split(g, 0.9, seed=0)

Both run on the device over the int32 COO lists (include/ngpde.h, "random graph sampling"; csrc/sampling.hip); there is no CPU
fallback.  Node positions are 0-based, as in graphops.py.  The random values come from a stateless Philox4x32-10: a result is a pure
function of the graph, the arguments and `seed`, the same bits on every run; `seed=None` draws the seed from torch's default CPU
generator, so `torch.manual_seed` governs it.

A result carries `edata["EID"]`, the int64 0-based COO positions of its edges in `g`.  Every edge feature and `edge_weight` follows
as in graphops.py: a float32 feature is moved by the library through an autograd function and keeps its gradient, a feature of another
dtype is indexed where it lives.  Where an edge can be drawn more than once (`replace=True`) the cotangents of its draws are summed
in draw order by the library's group reduce -- no float atomics anywhere.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, graphops
from .graphops import _arg_error, _coo, _device, _edge_weight_of, _f32_device, _Index, _is_f32, _new_graph, _node_index, _outer, _select_all
from .plans import _rows_index

_DIRS = {"out": 0, "in": 1}


def _seed_of(seed, what):
    if seed is None:
        return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise _arg_error(f"{what}: seed must be an integer or None, not {seed!r}")
    if not 0 <= int(seed) < 2 ** 64:
        raise _arg_error(f"{what}: seed {seed} outside 0 : 2^64 - 1")
    return int(seed)


class _Draws:
    """the draws of a sample with replacement grouped by the edge they name: ngpde_coo_coalesce of the pairs (0, EID) -- a stable radix
    (counting) sort, so the members of a group ascend by draw"""

    def __init__(self, eid, n_edges, dev):
        m = int(eid.numel())
        self.n_rows, self.copies = m, 1
        zero = torch.zeros(m, dtype=torch.int32, device=dev)
        s_out = torch.empty(m, dtype=torch.int32, device=dev)
        t_out = torch.empty(m, dtype=torch.int32, device=dev)
        self.group_ptr = torch.empty(m + 1, dtype=torch.int32, device=dev)
        self.member = torch.empty(m, dtype=torch.int32, device=dev)
        self.group_of = torch.empty(m, dtype=torch.int32, device=dev)
        n_out = C.c_int64(0)
        _lib.check(_lib.load().ngpde_coo_coalesce(max(n_edges, 1), m, _lib.ptr(zero), _lib.ptr(eid.to(torch.int32)), 0, 0, _lib.ptr(s_out),
                                                  _lib.ptr(t_out), _lib.ptr(self.group_ptr), _lib.ptr(self.member), _lib.ptr(self.group_of),
                                                  C.byref(n_out), _lib.current_stream()))
        self.n_groups = int(n_out.value)
        self.edges = t_out[:self.n_groups].to(torch.int64)          # the distinct drawn edges, ascending


class _RepeatedRowsFn(torch.autograd.Function):
    """x [outer][E] -> [outer][n_draws] by an index list that may repeat.  ngpde_rows_index's scatter needs distinct entries, so the
    pullback adds the cotangents of every edge's draws in draw order (ngpde_group_reduce_forward over the draws grouped by edge) and
    scatters the sums to the distinct drawn edges."""

    @staticmethod
    def forward(ctx, x, eid, n_edges):
        ctx.meta = (eid, n_edges)
        return _rows_index(x.detach(), eid, n_edges, False)

    @staticmethod
    def backward(ctx, dout):
        eid, n_edges = ctx.meta
        outer = dout.shape[0]
        if eid.numel() == 0 or outer == 0:
            return torch.zeros((outer, n_edges), dtype=torch.float32, device=dout.device), None, None
        draws = _Draws(eid, n_edges, dout.device)
        sums = graphops._GroupReduceFn.apply(dout.T, draws, _lib.AGGR["+"])          # [n_groups][outer]
        return _rows_index(sums.T.contiguous(), draws.edges, n_edges, True), None, None


def _select_repeated(v, index, n, dev):
    """v[..., index] where index may name an edge more than once"""
    if _is_f32(v):
        x = _f32_device(v, dev)
        rows = _RepeatedRowsFn.apply(x.reshape(_outer(x), n), index.dev, n)
        return rows.reshape(tuple(x.shape[:-1]) + (len(index),))
    if isinstance(v, torch.Tensor):
        return v[..., index.dev.to(v.device)]
    return np.asarray(v)[..., index.host()]


def _edge_parts(g, index, dev, repeated=False):
    """(edata with EID, edge_weight) of the edges `index` (an _Index of COO positions) of g"""
    w = _edge_weight_of(g)
    n = g.num_edges
    if repeated:
        edata = {k: _select_repeated(v, index, n, dev) for k, v in g.edata.items()}
        w = None if w is None else _select_repeated(w, index, n, dev).reshape(-1)
    else:
        edata = _select_all(g.edata, index, n, dev)
        w = None if w is None else graphops._select(w, index, n, dev).reshape(-1)
    edata["EID"] = index.dev
    return edata, w


def sample_neighbors(g, nodes=None, K=-1, *, dir="in", replace=False, dropnodes=False, seed=None):
    """[UPSTREAM GNNGraphs.sample_neighbors(g, nodes, K; dir, replace, dropnodes)] for every listed node (0-based, distinct; None: every
    node) a sample of its inbound (dir="in") or outbound ("out") edges; the graph on the same nodes that holds the sampled edges only.
    Edges of unlisted nodes are dropped.  K = -1 keeps every edge of a listed node, K = 0 none.

    replace=False: a uniform subset of min(K, deg) edges per node, in COO order.  The edge at COO position e has the key
    draw(seed, stream 1, counter e) and a node keeps the edges of its row with the smallest (key, e): what node v gets does not depend
    on which other nodes are listed.  replace=True: every listed node with an edge gets exactly K, draw j of node v being entry
    (draw(seed, stream 2, counter (v, j)) * deg) >> 64 of its row in COO order; the result lists them by listed node, then j.

    `edata["EID"]` holds the COO positions of the sampled edges in g; features and `edge_weight` follow (gradients included: with
    replace=True an edge's gradient is the sum over its draws).  Node data, graph_indicator and the locality order carry over.
    dropnodes=True keeps only the nodes that are an end of a sampled edge, ascending and relabelled, their old positions in
    `ndata["NID"]`."""
    what = "sample_neighbors"
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < -1:
        raise _arg_error(f"{what}: K must be an integer >= -1 (-1 keeps every edge), not {K!r}")
    if replace and K == -1:
        raise _arg_error(f"{what}: K = -1 (every edge) with replace=True; give the number of draws per node")
    code = _DIRS.get(dir) if isinstance(dir, str) else None
    if code is None:
        raise _arg_error(f"{what}: dir must be 'in' or 'out', not {dir!r}")
    seed = _seed_of(seed, what)
    dev = _device()
    s, t = _coo(g, dev)
    e, K = g.num_edges, int(K)
    listed = None if nodes is None else _node_index(nodes, dev)
    if listed is not None and len(listed) == 0:          # (the C entry reads an absent list as every node)
        listed, K = None, 0
    bound = (g.num_nodes if listed is None else len(listed)) * K if replace else e
    s_out = torch.empty(bound, dtype=torch.int32, device=dev)
    t_out = torch.empty(bound, dtype=torch.int32, device=dev)
    eid = torch.empty(bound, dtype=torch.int64, device=dev)
    n_out = C.c_int64(0)
    _lib.check(_lib.load().ngpde_coo_sample_neighbors(g.num_nodes, e, _lib.ptr(s), _lib.ptr(t), 0, code, 0 if listed is None else len(listed),
                                                      None if listed is None else _lib.ptr(listed.dev), K, int(bool(replace)), seed,
                                                      _lib.ptr(s_out), _lib.ptr(t_out), _lib.ptr(eid), C.byref(n_out), _lib.current_stream()))
    m = int(n_out.value)
    edata, w = _edge_parts(g, _Index(eid[:m]), dev, repeated=bool(replace))
    out = _new_graph(s_out[:m], t_out[:m], g.num_nodes, dev, num_graphs=g.num_graphs, indicator=g.graph_indicator, ndata=g.ndata, edata=edata,
                     gdata=g.gdata, edge_weight=w, order=g._shared.get("order"))
    if not dropnodes:
        return out
    ends = torch.nonzero(graphops.degree(out, "both", edge_weight=False) > 0).reshape(-1)          # ascending
    out = graphops.induced_subgraph(out, ends)
    out.ndata["NID"] = ends
    return out


def rand_edge_split(g, frac, *, bidirected=None, seed=None):
    """[UPSTREAM GNNGraphs.rand_edge_split(g, frac; bidirected)] a random partition of the edges: (g1, g2) on all the nodes of g, both
    in COO order, each with `edata["EID"]`, features and `edge_weight` following.

    bidirected=False: g1 holds the round(frac * E) edges with the smallest (key, e), the key of edge e being draw(seed, stream 3,
    counter e).  bidirected=True (the default where is_bidirected(g) holds): the key belongs to the unordered pair of ends, so both
    directions of a pair -- and parallel copies -- land on the same side; with P the number of edges with s <= t, g1 holds the pairs
    whose key is at most that of rank round(frac * P) - 1 among those edges.  bidirected=True on a graph that is not is an
    ArgumentError."""
    what = "rand_edge_split"
    try:
        frac = float(frac)
    except (TypeError, ValueError):
        raise _arg_error(f"{what}: frac must be a number in [0, 1], not {frac!r}") from None
    if not 0.0 <= frac <= 1.0:
        raise _arg_error(f"{what}: frac must lie in [0, 1], not {frac!r}")
    seed = _seed_of(seed, what)
    dev = _device()
    if bidirected is None:
        bidirected = graphops.is_bidirected(g)
    elif bidirected and not graphops.is_bidirected(g):
        raise _arg_error(f"{what}: bidirected=True on a graph that is not bidirected")
    s, t = _coo(g, dev)
    e = g.num_edges
    ranked = int(np.count_nonzero(g._s0 <= g._t0)) if bidirected else e
    n_first = int(round(frac * ranked))
    side = torch.empty(e, dtype=torch.int32, device=dev)
    kept = torch.empty((2, e), dtype=torch.int64, device=dev)
    n0 = C.c_int64(0)
    _lib.check(_lib.load().ngpde_coo_rand_split(g.num_nodes, e, _lib.ptr(s), _lib.ptr(t), 0, n_first, int(bool(bidirected)), seed, _lib.ptr(side),
                                                _lib.ptr(kept[0]), _lib.ptr(kept[1]), C.byref(n0), _lib.current_stream()))
    n0 = int(n0.value)
    parts = []
    for eid in (kept[0, :n0], kept[1, :e - n0]):
        edata, w = _edge_parts(g, _Index(eid), dev)
        parts.append(_new_graph(s[eid], t[eid], g.num_nodes, dev, num_graphs=g.num_graphs, indicator=g.graph_indicator, ndata=g.ndata,
                                edata=edata, gdata=g.gdata, edge_weight=w, order=g._shared.get("order")))
    return tuple(parts)
