"""Graph traversal: the questions whose answer needs a walk over the graph.  The reference's GNNGraph is a Graphs.AbstractGraph (`using
Graphs`, src/NeuralGraphPDE.jl:16; GNNGraphs re-exported at src/NeuralGraphPDE.jl:4), so upstream `connected_components(g)`,
`is_connected(g)`, `gdistances(g, sources)` and `neighborhood(g, v, d)` work on it directly:

    is_connected(radius_graph(p, r))                          # did the cloud fall apart at this radius?
    gb = split_components(g)                                  # a mesh file with several bodies as a batch, one member per body:
    laplacian_lambda_max(gb); cg_solve(L(gb), B)              # ... one null vector per COMPONENT, which the per-graph solvers need
    d = hop_distance(g, boundary_nodes)                       # the hop distance to the boundary: a node feature, and "do L layers reach?"
    patch = induced_subgraph(g, neighborhood(g, seeds, 3))    # the nodes within 3 hops: a sub-domain to train on
    sp = shortest_paths(g, boundary_nodes, edge_weight=lengths)   # the geodesic distance to the boundary along edges of length |x_s - x_t|

(the last is upstream `dijkstra_shortest_paths(g, srcs, distmx)`).  Node positions are 0-based, as in graphops.py.  Everything runs on
the device over the int32 COO lists (include/ngpde.h, "graph traversal"; csrc/graph_traverse.hip, csrc/graph_paths.hip); there is no
CPU fallback.  The components and hop distances are integers and their only atomics are integer min / or / add; the shortest paths
are float32 and use no atomics at all (synchronous rounds, fp32 addition is monotone): every result is bitwise equal from run to run
and depends neither on the launch geometry nor -- the parents of shortest_paths apart, which follow a stated row order -- on the COO order.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .graphops import _DIRS, _Index, _arg_error, _coo, _device, _edge_weight_of, _f32_device, _induced, _is_f32, _new_graph
from .matrices import _is_int
from .queries import _ids

__all__ = ["Components", "connected_components", "is_connected", "split_components", "hop_distance", "neighborhood", "ShortestPaths",
           "shortest_paths"]


def _check_every_arg(check_every):
    if not _is_int(check_every) or not 0 <= check_every < 2 ** 31:
        raise _arg_error(f"check_every must be an integer >= 0 (0: no read-back), not {check_every!r}")


def _bool_args(**flags):
    for name, flag in flags.items():
        if not isinstance(flag, (bool, np.bool_)):
            raise _arg_error(f"{name} must be a bool, not {flag!r}")


def _workspace(nbytes, dev):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def _rounds_args(max_rounds, check_every, what="max_rounds"):
    _check_every_arg(check_every)
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
        ws = _workspace(lib.ngpde_coo_components_workspace_bytes(n), dev)
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
    row entry; with_eid (ngpde_coo_rows_eid): the COO position of every row entry as well"""

    def __init__(self, g, code, dev, with_eid=False):
        s, t = _coo(g, dev)
        self.nnz = g.num_edges
        self.row_ptr = torch.empty(g.num_nodes + 1, dtype=torch.int32, device=dev)
        self.other = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        self.eid = torch.empty(self.nnz, dtype=torch.int32, device=dev) if with_eid else None
        lib = _lib.load()
        entry, eid = (lib.ngpde_coo_rows_eid, (_lib.ptr(self.eid),)) if with_eid else (lib.ngpde_coo_rows, ())
        _lib.check(entry(g.num_nodes, self.nnz, _lib.ptr(s), _lib.ptr(t), 0, code, _lib.ptr(self.row_ptr), _lib.ptr(self.other), *eid,
                         _lib.current_stream()))


def _row_sets(g, code, dev, with_eid=False):
    """(a, b): the rows plans a direction code walks, b None unless "both" -- following s -> t, a node is reached from the SOURCES of
    its incoming edges: the rows grouped by target.  A plan lives on `dev` with the structure, shared by every copy of the graph (as
    the key plan is), those with COO positions under a key of their own: a second call sorts nothing"""
    plans = []
    for c in ((1,), (0,), (1, 0))[code]:
        key = ("rows_eid" if with_eid else "rows", c, str(dev))
        if key not in g._shared:
            g._shared[key] = _RowsPlan(g, c, dev, with_eid)
        plans.append(g._shared[key])
    return plans[0], (plans[1] if len(plans) > 1 else None)


def _dir_code(dir):
    code = _DIRS.get(dir) if isinstance(dir, str) else None
    if code is None:
        raise _arg_error(f"dir must be 'out', 'in' or 'both', not {dir!r}")
    return code


def _hop_args(dir, max_hops, check_every, what="max_hops"):
    code = _dir_code(dir)
    if max_hops is not None and (not _is_int(max_hops) or not 0 <= max_hops < 2 ** 62):
        raise _arg_error(f"{what} must be an integer >= 0{'' if what == 'd' else ' (or None: no bound)'}, not {max_hops!r}")
    _check_every_arg(check_every)
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
    _bool_args(separate=separate)
    sources = _node_list(sources, "hop_distance: sources")
    dev = _device()
    src = _ids(sources, dev, "hop_distance: sources")
    lib, n, k = _lib.load(), g.num_nodes, int(src.numel())
    a, b = _row_sets(g, code, dev)
    dist = torch.empty((k, n) if separate else (n,), dtype=torch.int32, device=dev)
    ws = _workspace(lib.ngpde_csr_hop_distance_workspace_bytes(n), dev)
    _lib.check(lib.ngpde_csr_hop_distance(n, a.nnz, _lib.ptr(a.row_ptr), _lib.ptr(a.other), 0 if b is None else b.nnz,
                                          None if b is None else _lib.ptr(b.row_ptr), None if b is None else _lib.ptr(b.other), k, _lib.ptr(src), 0,
                                          int(bool(separate)), -1 if max_hops is None else int(max_hops), int(check_every), _lib.ptr(dist),
                                          _lib.ptr(ws), int(ws.numel()), _lib.current_stream()))
    return dist


class ShortestPaths:
    """[UPSTREAM Graphs.DijkstraState / BellmanFordState] what shortest_paths returns, on the device:
        dist         float32 [N], or [S, N] with separate=True: 0 at the sources, +inf where unreachable or farther than max_dist
        parent_eid   int32, shaped like dist (None without return_parents): the COO position of the tree edge into every node, -1
                     at sources and unreached nodes
        parents      int32, shaped like dist (None without return_parents): the node at the other end of that edge, -1 likewise
        flags        int32[2] on the device: [the rounds run, 1 if the last enqueued round still lowered a distance]
        rounds       the relaxation rounds run, the confirming one included (read from `flags` on first use)
        unfinished   did the distances still change after max_rounds rounds?  What a caller with check_every=0 asks instead of
                     catching NGPDE_ERR_STATE (read from `flags` on first use)"""

    def __init__(self, dist, parent_eid, parents, flags):
        self.dist, self.parent_eid, self.parents, self.flags = dist, parent_eid, parents, flags
        self._host_flags = self._host_parents = self._host_dist = None

    def _flags(self):
        if self._host_flags is None:
            self._host_flags = self.flags.cpu().numpy()
        return self._host_flags

    @property
    def rounds(self):
        return int(self._flags()[0])

    @property
    def unfinished(self):
        return bool(self._flags()[1])

    def __repr__(self):
        return f"ShortestPaths(dist {tuple(self.dist.shape)}{'' if self.parents is None else ', with parents'})"

    def path_to(self, v, row=0):
        """[UPSTREAM Graphs.enumerate_paths(state, v)] the nodes from the source to `v` along the tree, as a Python list; [] if `v`
        is unreached.  `row` picks the source with separate=True.  The parents are read to the host once and kept."""
        if self.parents is None:
            raise _arg_error("path_to needs the parents: call shortest_paths(..., return_parents=True)")
        rows = self.dist.shape[0] if self.dist.dim() == 2 else 1
        n = int(self.dist.shape[-1])
        if not _is_int(v) or not 0 <= v < n:
            raise _arg_error(f"path_to: v must be a node in 0 : {n - 1}, not {v!r}")
        if not _is_int(row) or not 0 <= row < rows:
            raise _arg_error(f"path_to: row must be in 0 : {rows - 1}, not {row!r}")
        if self._host_parents is None:
            self._host_parents = self.parents.reshape(rows, n).cpu().numpy()
            self._host_dist = self.dist.reshape(rows, n).cpu().numpy()
        if not np.isfinite(self._host_dist[row, v]):
            return []
        parent, path = self._host_parents[row], [int(v)]
        while parent[path[-1]] >= 0:
            path.append(int(parent[path[-1]]))
            if len(path) > n:
                raise _lib.NgpdeError(_lib.ERR_STATE, "path_to: the parents do not form a tree (were the rounds left unfinished?)")
        return path[::-1]


def _path_weights(g, edge_weight):
    """the weights in COO order -- the graph's own, or the E float32 values given -- or None: 1 per edge.  Checked on the host."""
    if edge_weight is None:
        return _edge_weight_of(g)
    w = edge_weight if isinstance(edge_weight, torch.Tensor) else np.asarray(edge_weight)
    if not _is_f32(w):
        raise _arg_error(f"shortest_paths: edge_weight must be float32, not {w.dtype}")
    if int(np.prod(tuple(w.shape))) != g.num_edges:
        raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                     f"DimensionMismatch: edge_weight has {int(np.prod(tuple(w.shape)))} entries for {g.num_edges} edges")
    return w


def shortest_paths(g, sources, edge_weight=None, dir="out", separate=False, max_dist=None, max_rounds=None, check_every=8,
                   return_parents=False):
    """[UPSTREAM Graphs.dijkstra_shortest_paths(g, srcs, distmx) / bellman_ford_shortest_paths] weighted shortest paths: a
    ShortestPaths on the device.  `dist` is float32, [N] -- the length of a shortest path from the NEAREST listed source -- or, with
    separate=True, [len(sources), N], one row per listed source; +inf where unreachable, 0 at the sources.  `sources`, `dir`,
    `separate`, batches (a source reaches only its own graph) and the errors for bad sources are hop_distance's.

    edge_weight=None takes the graph's own `edge_weight` if it has one, else 1 per edge; otherwise a float32 tensor / array of E
    weights in COO order -- for the geodesic distance along a mesh or a radius graph, the edge lengths |x_s - x_t| that apply_edges
    computes.  +inf and 0 are valid weights; a negative or NaN weight is an ArgumentError that names the smallest offending COO
    position (found on the device by the launch that gathers the weights into row order).  `max_dist` (a float >= 0, rounded to
    float32, or None): nodes farther than it get +inf; a node at exactly max_dist keeps its distance.  There is NO gradient to
    edge_weight (as upstream): it is read detached.

    Synchronous relaxation rounds (ngpde_csr_shortest_paths): a round sets d[v] = min(d[v], min over v's row of fl32(d[u] + w)) from
    the values of the round before only (two buffers alternate), one launch with a lane per node and group of sources that writes
    its own cells only -- no atomics; a hub's row is walked by a whole wave.  fp32 addition is monotone, so `dist` is a pure
    function of graph, weights and sources: bitwise what a float32 heap Dijkstra returns, whatever the COO order or the geometry.
    With return_parents=True `parent_eid` / `parents` name the tree edge into every node: recorded only when the distance strictly
    decreases, the first candidate in row order winning a tie (COO order inside a row; for dir="both" the edges into the node before
    those out of it), so they are a pure function of the COO list too, every parent edge is tight and the parents form a tree also
    with zero weights; `sp.path_to(v)` walks it.  separate=True runs ceil(S / 64) passes, one launch per round for all the sources
    of a pass.  The rows are sorted once per (graph, direction) and kept with the structure.

    Rounds are enqueued in groups of `check_every` with one read-back per group.  `max_rounds` (None: N, which always suffices
    with non-negative weights) bounds them: still changing after that many is an error (status NGPDE_ERR_STATE), never a partial
    answer.  check_every=0 needs max_rounds, enqueues exactly that many rounds and reads nothing back: once the rows plan exists,
    with `sources` an int64 and `edge_weight` a float32 device tensor, the call can be captured into a HIP graph; `sp.unfinished`
    then tells what the status would have (bad sources and weights are not raised there: nothing is relaxed through them)."""
    code = _dir_code(dir)
    _rounds_args(max_rounds, check_every)
    _bool_args(separate=separate, return_parents=return_parents)
    if max_dist is not None and (isinstance(max_dist, (bool, np.bool_)) or not isinstance(max_dist, (int, float, np.integer, np.floating))
                                 or not max_dist >= 0):
        raise _arg_error(f"max_dist must be a number >= 0 (or None: no bound), not {max_dist!r}")
    sources = _node_list(sources, "shortest_paths: sources")
    w = _path_weights(g, edge_weight)
    dev = _device()
    if w is not None:
        w = _f32_device(w, dev).detach().reshape(-1).contiguous()
    src = _ids(sources, dev, "shortest_paths: sources")
    lib, n, k = _lib.load(), g.num_nodes, int(src.numel())
    a, b = _row_sets(g, code, dev, with_eid=True)
    shape = (k, n) if separate else (n,)
    dist = torch.empty(shape, dtype=torch.float32, device=dev)
    parent_eid = torch.empty(shape, dtype=torch.int32, device=dev) if return_parents else None
    parents = torch.empty(shape, dtype=torch.int32, device=dev) if return_parents else None
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    ws = _workspace(lib.ngpde_csr_shortest_paths_workspace_bytes(n, a.nnz, 0 if b is None else b.nnz, k, int(bool(separate))), dev)
    none = (0, None, None, None)
    _lib.check(lib.ngpde_csr_shortest_paths(n, a.nnz, _lib.ptr(a.row_ptr), _lib.ptr(a.other), _lib.ptr(a.eid),
                                            *(none if b is None else (b.nnz, _lib.ptr(b.row_ptr), _lib.ptr(b.other), _lib.ptr(b.eid))), k,
                                            _lib.ptr(src), 0, int(bool(separate)), _lib.ptr(w), float("inf") if max_dist is None else float(max_dist),
                                            0 if max_rounds is None else int(max_rounds), int(check_every), _lib.ptr(dist), _lib.ptr(parent_eid),
                                            _lib.ptr(parents), _lib.ptr(flags), _lib.ptr(ws), int(ws.numel()), _lib.current_stream()))
    return ShortestPaths(dist, parent_eid, parents, flags)


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
