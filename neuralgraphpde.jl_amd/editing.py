"""Graph editing and negative sampling: the transforms of the GNNGraphs re-export (src/NeuralGraphPDE.jl:4 of the reference) that
CHANGE a graph -- `add_nodes`, `add_edges`, `remove_edges`, `remove_nodes`, `to_unidirected`, `set_edge_weight` / `get_edge_weight` --
and `negative_sample`: a point cloud refined or coarsened between two `updategraph` calls, a boundary cut, the non-edges an edge
predictor trains against:

    g = remove_nodes(g, boundary)                                  # cut
    g = add_edges(add_nodes(g, 2, ndata=x_new), [n, n + 1], [0, 1])           # refine
    st = updategraph(st, g)
    neg = negative_sample(g, seed=epoch)                           # as many non-edges as g has edges

Node positions and edge (COO) positions are 0-based, as in graphops.py.  Everything runs on the device over the int32 COO lists
(include/ngpde.h, "graph editing"; csrc/graph_edit.hip); there is no CPU fallback.  A result is a new GNNGraph whose device COO lists
are already in place, so its handle builds without an upload; where the node set is unchanged the source's cached locality order is kept.

Features follow as in graphops.py: a float32 feature or `edge_weight` is moved (ngpde_rows_index) or reduced (ngpde_group_reduce_*) by
the library through autograd functions, or concatenated on the device, and keeps its gradient; a feature of another dtype is indexed
or concatenated where it lives and keeps dtype and placement.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, graphops
from .graphops import _arg_error, _coo, _device, _edge_weight_of, _f32_device, _Index, _is_f32, _new_graph, _node_index, _select, _select_all
from .graphs import GNNGraph
from .sampling import _seed_of


def _count(v, what, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
        raise _arg_error(f"{what}: {name} must be a non-negative integer, not {v!r}")
    return int(v)


def _new_data(given, have, default, n_new, what, kind):
    """the features of the new nodes / edges under the keys the graph has: every key, nothing else, last dimension n_new"""
    if given is None:
        given = {}
    elif not isinstance(given, dict):
        given = {default: given}
    if set(given) != set(have):
        raise _arg_error(f"{what}: the graph has the {kind} features {sorted(have)}, the new {kind}s bring {sorted(given)}; "
                         "they must bring the same keys")
    for k, v in given.items():
        shape = tuple(v.shape) if hasattr(v, "shape") else tuple(np.asarray(v).shape)
        if len(shape) == 0 or shape[-1] != n_new:
            raise _arg_error(f"{what}: {kind} feature '{k}' has size {shape}, its last dimension must be {n_new}")
        if shape[:-1] != tuple(have[k].shape[:-1]):
            raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, f"DimensionMismatch: {what}: {kind} feature '{k}' has size {shape}, "
                                         f"the graph's has {tuple(have[k].shape)}")
    return given


def _cat(old, new, dev):
    """[old, new] along the last dimension: float32 on the device (with its gradient), anything else where `old` lives, in its dtype"""
    if _is_f32(old):
        return torch.cat([_f32_device(old, dev), _f32_device(new, dev)], dim=-1)
    if isinstance(old, torch.Tensor):
        new = new if isinstance(new, torch.Tensor) else torch.as_tensor(np.asarray(new))
        return torch.cat([old, new.to(old.device, old.dtype)], dim=-1)
    new = new.detach().cpu().numpy() if isinstance(new, torch.Tensor) else np.asarray(new)
    return np.concatenate([np.asarray(old), new.astype(np.asarray(old).dtype)], axis=-1)


def _ends(v, dev):
    """node positions as an int32 device list; what does not fit int32 is out of every node range and stays so"""
    t = v.reshape(-1).to(dev) if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.int64).reshape(-1), device=dev)
    return t.to(torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()


# ---- nodes ----------------------------------------------------------------------------------------------------------------------


def add_nodes(g, n, ndata=None):
    """[UPSTREAM GNNGraphs.add_nodes(g, n; ndata...)] g with n >= 0 isolated nodes appended (positions N .. N + n - 1); the edges, their
    features and the graph features are unchanged.  If g has node features, `ndata` (a dict, or a bare array for the key "x") must give
    every key with last dimension n; they are appended.  A batch (g.num_graphs > 1) is refused: the new nodes would belong to no graph.
    The cached locality order is dropped, because the node set changed."""
    what = "add_nodes"
    n = _count(n, what, "n")
    if g.num_graphs > 1:
        raise _arg_error(f"{what}: the graph is a batch of {g.num_graphs} graphs; the new nodes would belong to none of them")
    new = _new_data(ndata, g.ndata, "x", n, what, "node")
    dev = _device()
    s, t = _coo(g, dev)
    return _new_graph(s, t, g.num_nodes + n, dev, num_graphs=g.num_graphs, indicator=None, ndata={k: _cat(v, new[k], dev) for k, v in g.ndata.items()},
                      edata=g.edata, gdata=g.gdata, edge_weight=g.edge_weight)


def remove_nodes(g, nodes):
    """[UPSTREAM GNNGraphs.remove_nodes(g, nodes)] g without the listed nodes (0-based; repeats allowed; an entry out of range is an
    ArgumentError): induced_subgraph on the ascending complement of `nodes`, so the remaining nodes keep their order and are renumbered,
    an edge stays iff both its ends do, and features and the graph indicator follow.  The number of graphs is kept even if one becomes
    empty."""
    dev = _device()
    listed = _node_index(nodes, dev)
    rest = torch.empty(g.num_nodes, dtype=torch.int64, device=dev)
    n_out = C.c_int64(0)
    _lib.check(_lib.load().ngpde_coo_complement_nodes(g.num_nodes, len(listed), _lib.ptr(listed.dev), _lib.ptr(rest), C.byref(n_out),
                                                      _lib.current_stream()))
    k = int(n_out.value)
    if k > 0:
        return graphops.induced_subgraph(g, rest[:k])
    none = _Index(rest[:0])          # nothing is left: no list for ngpde_coo_compact to relabel by
    w = _edge_weight_of(g)
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    return _new_graph(empty, empty.clone(), 0, dev, num_graphs=g.num_graphs,
                      indicator=None if g.graph_indicator is None else g.graph_indicator[:0], ndata=_select_all(g.ndata, none, g.num_nodes, dev),
                      edata=_select_all(g.edata, none, g.num_edges, dev), gdata=g.gdata,
                      edge_weight=None if w is None else _select(w, none, g.num_edges, dev).reshape(-1))


# ---- edges ----------------------------------------------------------------------------------------------------------------------


def add_edges(g, s, t, edata=None, edge_weight=None):
    """[UPSTREAM GNNGraphs.add_edges(g, s, t; edata)] g with the edges (s[k], t[k]) appended (0-based ends): the old edges in order, then
    the new ones in the order given.  If g has edge features or an `edge_weight`, the new edges must bring the same keys (`edata`: a
    dict, or a bare array for the key "e"; `edge_weight`: one weight per new edge).  A new end outside 0 : N - 1 is a
    DimensionMismatch; on a batch, a new edge whose ends lie in different graphs is an ArgumentError.  Both are found on the device
    by the launch that concatenates the lists."""
    what = "add_edges"
    w = _edge_weight_of(g)
    n_s = int(np.prod(tuple(s.shape))) if hasattr(s, "shape") else len(s)
    n_t = int(np.prod(tuple(t.shape))) if hasattr(t, "shape") else len(t)
    if n_s != n_t:
        raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, f"DimensionMismatch: {what}: s has {n_s} entries, t has {n_t}")
    new = _new_data(edata, g.edata, "e", n_s, what, "edge")
    if (w is None) != (edge_weight is None):
        raise _arg_error(f"{what}: the graph has {'an' if w is not None else 'no'} edge_weight, the new edges bring "
                         f"{'one' if edge_weight is not None else 'none'}; they must bring the same keys")
    if edge_weight is not None and int(np.prod(tuple(edge_weight.shape))) != n_s:
        raise _arg_error(f"{what}: edge_weight has {int(np.prod(tuple(edge_weight.shape)))} entries for {n_s} new edges")
    dev = _device()
    s0, t0 = _coo(g, dev)
    s1, t1 = _ends(s, dev), _ends(t, dev)
    gi = None if g.graph_indicator is None else torch.as_tensor(np.ascontiguousarray(g.graph_indicator, dtype=np.int32), device=dev)
    m = g.num_edges + n_s
    s_out = torch.empty(m, dtype=torch.int32, device=dev)
    t_out = torch.empty(m, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().ngpde_coo_append(g.num_nodes, g.num_edges, _lib.ptr(s0), _lib.ptr(t0), 0, n_s, _lib.ptr(s1), _lib.ptr(t1),
                                            _lib.ptr(gi), _lib.ptr(s_out), _lib.ptr(t_out), _lib.current_stream()))
    if w is not None:
        w = _cat(w.reshape(-1), edge_weight.reshape(-1), dev)
    return _new_graph(s_out, t_out, g.num_nodes, dev, num_graphs=g.num_graphs, indicator=g.graph_indicator, ndata=g.ndata,
                      edata={k: _cat(v, new[k], dev) for k, v in g.edata.items()}, gdata=g.gdata, edge_weight=w, order=g._shared.get("order"))


def remove_edges(g, s, t=None):
    """[UPSTREAM GNNGraphs.remove_edges(g, edges) / (g, s, t)] g without some edges; the kept ones stay in COO order, features and
    `edge_weight` follow them.

    remove_edges(g, edges): `edges` lists COO positions (0-based); repeats are allowed, an entry outside 0 : E - 1 is an ArgumentError.
    remove_edges(g, s, t): every edge whose (source, target) equals a listed pair goes, all its parallel copies included; a listed
    pair that g does not have is ignored, a listed end outside the node range is an ArgumentError."""
    what = "remove_edges"
    w = _edge_weight_of(g)
    dev = _device()
    s0, t0 = _coo(g, dev)
    e = g.num_edges
    positions = ls = lt = None
    if t is None:
        positions = _node_index(s, dev).dev
        n_listed = int(positions.numel())
    else:
        ls, lt = _ends(s, dev), _ends(t, dev)
        n_listed = int(ls.numel())
        if int(lt.numel()) != n_listed:
            raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, f"DimensionMismatch: {what}: s has {n_listed} entries, t has {int(lt.numel())}")
    s_out = torch.empty(e, dtype=torch.int32, device=dev)
    t_out = torch.empty(e, dtype=torch.int32, device=dev)
    kept = torch.empty(e, dtype=torch.int64, device=dev)
    n_out = C.c_int64(0)
    _lib.check(_lib.load().ngpde_coo_remove_edges(g.num_nodes, e, _lib.ptr(s0), _lib.ptr(t0), 0, n_listed, _lib.ptr(positions), _lib.ptr(ls),
                                                  _lib.ptr(lt), _lib.ptr(s_out), _lib.ptr(t_out), _lib.ptr(kept), C.byref(n_out),
                                                  _lib.current_stream()))
    k = int(n_out.value)
    kept = _Index(kept[:k])
    return _new_graph(s_out[:k], t_out[:k], g.num_nodes, dev, num_graphs=g.num_graphs, indicator=g.graph_indicator, ndata=g.ndata,
                      edata=_select_all(g.edata, kept, e, dev), gdata=g.gdata,
                      edge_weight=None if w is None else _select(w, kept, e, dev).reshape(-1), order=g._shared.get("order"))


def to_unidirected(g):
    """[UPSTREAM GNNGraphs.to_unidirected] every edge turned into (min(s, t), max(s, t)), then coalesced exactly as to_bidirected does:
    one edge per distinct pair, ordered by source, then target, `edge_weight` and every float32 edge feature the mean over the pair's
    copies in ascending COO position.  Self loops stay."""

    def oriented(dev):
        s, t = _coo(g, dev)
        s_out, t_out = torch.empty_like(s), torch.empty_like(t)
        _lib.check(_lib.load().ngpde_coo_orient(g.num_nodes, g.num_edges, _lib.ptr(s), _lib.ptr(t), _lib.ptr(s_out), _lib.ptr(t_out),
                                                _lib.current_stream()))
        return s_out, t_out

    return graphops._coalesce(g, "mean", False, "to_unidirected", coo=oriented)


def set_edge_weight(g, w):
    """[UPSTREAM GNNGraphs.set_edge_weight(g, w)] a copy of g with the edge weight w (one entry per edge; a wrong length is a
    DimensionMismatch).  The structure, and with it the native handles, is shared."""
    if w is None or not hasattr(w, "shape"):
        w = np.asarray([] if w is None else w, dtype=np.float32)
    if int(np.prod(tuple(w.shape))) != g.num_edges:
        raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                     f"DimensionMismatch: set_edge_weight: w has {int(np.prod(tuple(w.shape)))} entries for {g.num_edges} edges")
    return GNNGraph(g, edge_weight=w)


def get_edge_weight(g):
    """[UPSTREAM GNNGraphs.get_edge_weight(g)] the graph's edge weight, or None"""
    return g.edge_weight


# ---- negative sampling ----------------------------------------------------------------------------------------------------------


def negative_sample(g, num_neg_edges=None, *, bidirected=None, seed=None):
    """[UPSTREAM GNNGraphs.negative_sample(g; num_neg_edges, bidirected)] a graph on the nodes of g, without features, whose
    `num_neg_edges` edges (default: g.num_edges) are NOT edges of g.  It never contains a self loop -- a deliberate difference from
    upstream, which can draw one.  bidirected (default: is_bidirected(g)): the result holds num_neg_edges // 2 unordered pairs {a, b},
    neither (a, b) nor (b, a) an edge of g, as the edges [a; b] followed by [b; a].  seed: as in sampling.py (None draws it from torch's
    default CPU generator).

    The result is a pure function of (graph, arguments, seed).  With U = N (N - 1), candidate j = 0, 1, 2, ... has the code
    c_j = (draw(seed, stream 4, counter (lo32 j, hi32 j)) * U) >> 64, which decodes as a = c // (N - 1), b' = c % (N - 1),
    b = b' + (b' >= a); with bidirected the pair is then made (min, max).  A candidate is a negative if it is not an edge of g (with
    bidirected: in neither direction).  The result is the first n_target distinct negatives of that sequence, in sequence order --
    whatever chunks the library walks the sequence in.  Every code is equally likely up to the bias of the multiply-high, which is
    at most U / 2^64 (U < 2^62), so the result is a uniform sample without replacement of the non-edges.

    With K the number of distinct non-loop pairs of g (unordered with bidirected) and U_eff = U (U / 2 with bidirected), asking for
    more than U_eff - K is an ArgumentError.  The walk stops with an NgpdeError after 64 * ceil(U_eff / (U_eff - K)) * (n_target + 16)
    candidates -- far beyond the U_eff * ln(U_eff - K) that collecting every non-edge takes -- and never truncates silently."""
    what = "negative_sample"
    num = g.num_edges if num_neg_edges is None else _count(num_neg_edges, what, "num_neg_edges")
    seed = _seed_of(seed, what)
    dev = _device()
    if bidirected is None:
        bidirected = graphops.is_bidirected(g)
    n_target = num // 2 if bidirected else num
    m = 2 * n_target if bidirected else n_target
    s, t = _coo(g, dev)
    s_out = torch.empty(m, dtype=torch.int32, device=dev)
    t_out = torch.empty(m, dtype=torch.int32, device=dev)
    n_out = C.c_int64(0)
    _lib.check(_lib.load().ngpde_coo_negative_sample(g.num_nodes, g.num_edges, _lib.ptr(s), _lib.ptr(t), 0, n_target, int(bool(bidirected)), seed,
                                                     0, _lib.ptr(s_out), _lib.ptr(t_out), C.byref(n_out), _lib.current_stream()))
    if int(n_out.value) != m:
        raise _lib.NgpdeError(_lib.ERR_STATE, f"{what}: the library wrote {int(n_out.value)} of {m} edges")
    return _new_graph(s_out, t_out, g.num_nodes, dev, num_graphs=g.num_graphs, indicator=g.graph_indicator, ndata=None, edata=None, gdata=None,
                      edge_weight=None, order=g._shared.get("order"))
