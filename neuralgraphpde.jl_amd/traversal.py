"""Graph traversal: the questions whose answer needs a walk over the graph.  The reference's GNNGraph is a Graphs.AbstractGraph (`using
Graphs`, src/NeuralGraphPDE.jl:16; GNNGraphs re-exported at src/NeuralGraphPDE.jl:4), so upstream `connected_components(g)`,
`is_connected(g)`, `gdistances(g, sources)` and `neighborhood(g, v, d)` work on it directly:

    is_connected(radius_graph(p, r))                          # did the cloud fall apart at this radius?
    gb = split_components(g)                                  # a mesh file with several bodies as a batch, one member per body:
    laplacian_lambda_max(gb); cg_solve(L(gb), B)              # ... one null vector per COMPONENT, which the per-graph solvers need
    d = hop_distance(g, boundary_nodes)                       # the hop distance to the boundary: a node feature, and "do L layers reach?"
    patch = induced_subgraph(g, neighborhood(g, seeds, 3))    # the nodes within 3 hops: a sub-domain to train on

Node positions are 0-based, as in graphops.py.  Everything runs on the device over the int32 COO lists (include/ngpde.h, "graph
traversal"; csrc/graph_traverse.hip); there is no CPU fallback.  The results are integers and the only atomics are integer min / or /
add: every result is bitwise equal from run to run and depends neither on the COO order nor on the launch geometry.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .graphops import _DIRS, _Index, _arg_error, _coo, _device, _induced, _new_graph
from .matrices import _is_int
from .queries import _ids

__all__ = ["Components", "connected_components", "is_connected", "split_components", "hop_distance", "neighborhood"]


def _rounds_args(max_rounds, check_every, what="max_rounds"):
    if not _is_int(check_every) or not 0 <= check_every < 2 ** 31:
        raise _arg_error(f"check_every must be an integer >= 0 (0: no read-back), not {check_every!r}")
    if max_rounds is not None and (not _is_int(max_rounds) or not 1 <= max_rounds < 2 ** 31):
        raise _arg_error(f"{what} must be an integer >= 1 (or None: the library's choice), not {max_rounds!r}")
    if check_every == 0 and max_rounds is None:
        raise _arg_error(f"check_every=0 enqueues exactly {what} rounds without a read-back: {what} must be given")


def _label(n, e, s, t, index_base, max_rounds, check_every, labels=None, rounds=None, ws=None):
    """ngpde_coo_components over device int32 lists: (labels, rounds) -- the smallest member of every node's component and the device
    words [rounds run, still hooking].  With the three buffers given and check_every=0 the call allocates nothing and reads nothing
    back: it can be captured into a HIP graph."""
    lib = _lib.load()
    dev = s.device if s is not None else _device()
    if labels is None:
        labels = torch.empty(n, dtype=torch.int32, device=dev)
    if rounds is None:
        rounds = torch.empty(2, dtype=torch.int32, device=dev)
    if ws is None:
        ws = torch.empty(int(lib.ngpde_coo_components_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    _lib.check(lib.ngpde_coo_components(n, e, _lib.ptr(s), _lib.ptr(t), index_base, 0 if max_rounds is None else int(max_rounds), int(check_every),
                                        _lib.ptr(labels), _lib.ptr(rounds), _lib.ptr(ws), int(ws.numel()), _lib.current_stream()))
    return labels, rounds


class Components:
    """[UPSTREAM Graphs.connected_components: Vector{Vector{Int}}] the weakly connected components of a graph, on the device, ranked by
    their smallest member:
        labels      int32[N]: the rank of every node's component
        smallest    int32[N]: the smallest member of every node's component
        count       the number of components;  sizes int32[count]
        ptr, order  the nodes grouped by component and ascending inside it, ragged like AdjacencyList: component k is
                    order[ptr[k] : ptr[k + 1]], which is also `comps[k]`
        per_graph   int32[num_graphs]: the components of every graph of a batch
        rounds      the hook-and-compress rounds the labelling took, the confirming one included
    `len(comps)` is count, `comps.tolist()` the components as Python lists."""

    def __init__(self, labels, smallest, count, sizes, ptr, order, per_graph, rounds):
        self.labels, self.smallest, self.count, self.sizes, self.ptr, self.order = labels, smallest, count, sizes, ptr, order
        self.per_graph, self.rounds = per_graph, rounds
        self._host_ptr = None

    def _bounds(self):
        if self._host_ptr is None:
            self._host_ptr = self.ptr.cpu().numpy()
        return self._host_ptr

    def __len__(self):
        return self.count

    def __getitem__(self, k):
        if not _is_int(k):
            raise TypeError(f"component positions are integers, not {type(k).__name__}")
        if not -self.count <= k < self.count:
            raise IndexError(f"component {k} of {self.count}")
        p = self._bounds()
        k = int(k) % self.count
        return self.order[int(p[k]):int(p[k + 1])]

    def __iter__(self):
        return (self[k] for k in range(self.count))

    def __repr__(self):
        return f"Components({self.count} components of {int(self.labels.numel())} nodes)"

    def tolist(self):
        p, o = self._bounds(), self.order.cpu().numpy()
        return [o[p[k]:p[k + 1]].tolist() for k in range(self.count)]


def connected_components(g, max_rounds=None, check_every=4):
    """[UPSTREAM Graphs.connected_components(g)] the weakly connected components (the edges seen as undirected): a Components on the
    device.  Self loops, parallel edges, isolated nodes and a graph without edges are valid.

    Root hooking with compression (ngpde_coo_components): a round hooks, per edge, the larger of the two ends' roots under the
    smaller with an integer atomicMin and then brings every node to its root by path halving; the first round that hooks nothing
    ends it.  A path of N nodes takes a handful of rounds however it is numbered, where neighbour-to-neighbour label propagation
    would take up to N - 1.  Rounds are enqueued in groups of `check_every` with one read-back per group; check_every=0 enqueues
    exactly `max_rounds` rounds and reads back once, at the end.  `max_rounds` (None: 2 * ceil(log2(max(N, 2))) + 8, in whole groups)
    bounds the rounds: still hooking after that many is an error (status NGPDE_ERR_STATE), never a partial answer.  The labels are a
    pure function of the edge set: neither the COO order, the launch geometry nor check_every changes them."""
    _rounds_args(max_rounds, check_every)
    gi = g.graph_indicator
    if g.num_graphs > 1 and gi is None:
        raise _arg_error(f"the graph holds {g.num_graphs} graphs but no graph_indicator: build it with batch(), radius_graph / "
                         "knn_graph(..., graph_indicator=) or GNNGraph(..., graph_indicator=)")
    dev = _device()
    lib = _lib.load()
    s, t = _coo(g, dev)
    n = g.num_nodes
    smallest, rounds = _label(n, g.num_edges, s, t, 0, max_rounds, check_every)
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    rank, sizes, order, ptr, per_graph = i32(n), i32(n), i32(n), i32(n + 1), i32(g.num_graphs)
    graph_of = None if gi is None else torch.as_tensor(np.ascontiguousarray(gi, dtype=np.int32), device=dev)
    count = C.c_int64(0)
    _lib.check(lib.ngpde_components_rank(n, _lib.ptr(smallest), g.num_graphs, _lib.ptr(graph_of), _lib.ptr(rank), _lib.ptr(sizes), _lib.ptr(order),
                                         _lib.ptr(ptr), C.byref(count), _lib.ptr(per_graph), _lib.current_stream()))
    r = rounds.cpu().numpy()
    if check_every == 0 and r[1]:
        raise _lib.NgpdeError(_lib.ERR_STATE, f"connected_components: still hooking after max_rounds = {max_rounds} rounds: the labels are "
                                              "not final (raise max_rounds)")
    k = int(count.value)
    return Components(rank, smallest, k, sizes[:k], ptr[:k + 1], order, per_graph, int(r[0]))


def is_connected(g):
    """[UPSTREAM Graphs.is_connected(g)] is every node reachable from every other, the edges seen as undirected?  A Python bool for one
    graph; for a batch a bool device tensor, one value per graph.  A graph without nodes is an ArgumentError."""
    if g.num_graphs > 1 and g.graph_indicator is not None:
        empty = np.flatnonzero(np.bincount(g.graph_indicator, minlength=g.num_graphs) == 0)
        if empty.size:
            raise _arg_error(f"is_connected: graph {int(empty[0])} of the batch has no nodes")
    elif g.num_nodes == 0:
        raise _arg_error("is_connected: the graph has no nodes")
    comps = connected_components(g)
    return comps.count == 1 if g.num_graphs == 1 else comps.per_graph == 1


def split_components(g):
    """the same graph with its nodes regrouped by component -- node k of the result is node `order[k]` of g (induced_subgraph's primitive
    with the full permutation: node and edge features and `edge_weight` follow with their gradients, edges stay in COO order) -- as
    a batch whose members are the components: num_graphs = count and a non-decreasing graph_indicator, which is what
    laplacian_lambda_max and cg_solve ask of a batch.  `ndata["NID"]` holds the int64 position in g of every node.  On a batch the
    components are ranked within the batch, which orders them by graph, because the members of a batch are contiguous.  Graph
    features are per graph of g and do not carry over."""
    comps = connected_components(g)
    dev = comps.order.device
    nodes = _Index(comps.order.to(torch.int64))
    p = _induced(g, nodes, dev)
    indicator = comps.labels.cpu().numpy()[nodes.host()] if comps.count > 1 else None
    ndata = dict(p.pop("ndata"))
    ndata["NID"] = nodes.dev
    return _new_graph(p.pop("s"), p.pop("t"), p.pop("n"), p.pop("dev"), num_graphs=max(comps.count, 1), indicator=indicator, ndata=ndata,
                      gdata=None, **p)


class _RowsPlan:
    """what ngpde_coo_rows wrote: the structure's rows grouped by source (code 0) or target (1) and the 0-based other end of every
    row entry"""

    def __init__(self, g, code, dev):
        s, t = _coo(g, dev)
        self.nnz = g.num_edges
        self.row_ptr = torch.empty(g.num_nodes + 1, dtype=torch.int32, device=dev)
        self.other = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().ngpde_coo_rows(g.num_nodes, self.nnz, _lib.ptr(s), _lib.ptr(t), 0, code, _lib.ptr(self.row_ptr), _lib.ptr(self.other),
                                              _lib.current_stream()))


def _rows_plan(g, code, dev):
    """the structure's rows on `dev`, shared by every copy of the graph (as the key plan is): a second call sorts nothing"""
    key = ("rows", code, str(dev))
    p = g._shared.get(key)
    if p is None:
        p = g._shared[key] = _RowsPlan(g, code, dev)
    return p


def _hop_args(dir, max_hops, check_every, what="max_hops"):
    code = _DIRS.get(dir) if isinstance(dir, str) else None
    if code is None:
        raise _arg_error(f"dir must be 'out', 'in' or 'both', not {dir!r}")
    if max_hops is not None and (not _is_int(max_hops) or not 0 <= max_hops < 2 ** 62):
        raise _arg_error(f"{what} must be an integer >= 0{'' if what == 'd' else ' (or None: no bound)'}, not {max_hops!r}")
    if not _is_int(check_every) or not 0 <= check_every < 2 ** 31:
        raise _arg_error(f"check_every must be an integer >= 0 (0: no read-back), not {check_every!r}")
    if check_every == 0 and max_hops is None:
        raise _arg_error("check_every=0 enqueues exactly max_hops levels without a read-back: max_hops must be given")
    return code


def _node_list(v, what):
    """an int or an integer sequence / tensor, refused here -- before any device call -- if it holds anything but integers"""
    if _is_int(v):
        return [int(v)]
    if isinstance(v, torch.Tensor):
        if v.dtype == torch.bool or v.is_floating_point() or v.is_complex():
            raise _arg_error(f"{what} must hold integers, not {v.dtype}")
        return v
    a = np.asarray(v)
    if a.dtype == np.bool_ or (not np.issubdtype(a.dtype, np.integer) and (a.size or a.dtype == object)):
        raise _arg_error(f"{what} must hold integers, not {a.dtype}")
    return a


def hop_distance(g, sources, dir="out", max_hops=None, separate=False, check_every=8):
    """[UPSTREAM Graphs.gdistances(g, sources)] hop distances (breadth-first levels): an int32 device tensor.  With separate=False its
    shape is [N] and every value the number of edges on a shortest path from the NEAREST listed source, following the edges s -> t
    (dir="out"), against them ("in") or either way ("both").  With separate=True the shape is [len(sources), N], one row per listed
    source in the order given (a source listed twice gives two equal rows).  Unreachable nodes, and nodes beyond `max_hops`, get -1;
    no sources give -1 everywhere.  On a batch a source only reaches its own graph.  `sources` is an int or an integer sequence /
    tensor of 0-based nodes; one outside 0 : N - 1 is a DimensionMismatch that names it.

    A level-synchronous pull on 64-bit source masks (ngpde_csr_hop_distance): one launch per level with a lane per node, which ORs
    the frontier words of the other ends of its row and writes its own node only -- no atomics, the same bits whatever the geometry;
    a hub's row is walked by a whole wave.  separate=True runs ceil(S / 64) passes of 64 sources each.  The by-node rows are sorted
    once per (graph, direction) and kept with the structure.  Levels are enqueued in groups of `check_every` with one read-back per
    group; with check_every=0 and a given max_hops exactly max_hops levels are enqueued and nothing is read back: once the rows
    plan exists and `sources` is an int64 device tensor the call can be captured into a HIP graph (a bad source is not raised
    there: it reaches nothing)."""
    code = _hop_args(dir, max_hops, check_every)
    if not isinstance(separate, (bool, np.bool_)):
        raise _arg_error(f"separate must be a bool, not {separate!r}")
    sources = _node_list(sources, "hop_distance: sources")
    dev = _device()
    src = _ids(sources, dev, "hop_distance: sources")
    lib, n, k = _lib.load(), g.num_nodes, int(src.numel())
    # following s -> t, a node is reached from the SOURCES of its incoming edges: the rows grouped by target
    plans = [_rows_plan(g, c, dev) for c in ((1,), (0,), (1, 0))[code]]
    a, b = plans[0], (plans[1] if len(plans) > 1 else None)
    dist = torch.empty((k, n) if separate else (n,), dtype=torch.int32, device=dev)
    nbytes = int(lib.ngpde_csr_hop_distance_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.ngpde_csr_hop_distance(n, a.nnz, _lib.ptr(a.row_ptr), _lib.ptr(a.other), 0 if b is None else b.nnz,
                                          None if b is None else _lib.ptr(b.row_ptr), None if b is None else _lib.ptr(b.other), k, _lib.ptr(src), 0,
                                          int(bool(separate)), -1 if max_hops is None else int(max_hops), int(check_every), _lib.ptr(dist),
                                          _lib.ptr(ws), nbytes, _lib.current_stream()))
    return dist


def neighborhood(g, nodes, d, dir="out"):
    """[UPSTREAM Graphs.neighborhood(g, v, d; dir)] the nodes within `d` hops of any listed node, the listed nodes included: an int64
    device tensor, ascending -- hop_distance(g, nodes, dir, max_hops=d) and the stable compaction of the reached nodes
    (ngpde_hop_reached_nodes).  It is what induced_subgraph takes: `induced_subgraph(g, neighborhood(g, seeds, 3))`."""
    _hop_args(dir, d, 8, what="d")
    if d is None:
        raise _arg_error("d must be an integer >= 0, not None")
    dist = hop_distance(g, nodes, dir=dir, max_hops=d)
    n = g.num_nodes
    out = torch.empty(n, dtype=torch.int64, device=dist.device)
    count = C.c_int64(0)
    _lib.check(_lib.load().ngpde_hop_reached_nodes(n, _lib.ptr(dist), 0, _lib.ptr(out), C.byref(count), _lib.current_stream()))
    return out[:int(count.value)]
