"""Graph queries and transforms: the part of GNNGraphs the reference re-exports (src/NeuralGraphPDE.jl:4) that a script uses between
making a graph and handing it to `updategraph` -- `degree`, `has_self_loops`, `has_multi_edges`, `is_bidirected`, `add_self_loops`,
`remove_self_loops`, `remove_multi_edges`, `to_bidirected`, `induced_subgraph`, `getgraph`, `unbatch`:

    g = to_bidirected(GNNGraph(tri_s, tri_t, num_nodes=n, index_base=0))    # docs/src/tutorials/VMH.md:53-55: mesh neighbours
    st = updategraph(st, g)
    ...
    members = unbatch(gb)                                                   # the inverse of batch()

Node and graph positions are 0-based here (`unbatch(g)[i]`, `getgraph(g, i)`, `induced_subgraph(g, nodes)`); `GNNGraph(s, t)` keeps its
`index_base` keyword.  Everything runs on the device over the int32 COO lists (include/ngpde.h, "graph queries and transforms";
csrc/graph_ops.hip); there is no CPU fallback.  A result is a new GNNGraph whose device COO lists are already in place, so its handle
builds without an upload; where the node set is unchanged the source's cached locality order is kept.

Features: a float32 feature is moved (ngpde_rows_index) or reduced (ngpde_group_reduce_*) by the library, through autograd functions --
a feature or edge_weight that requires grad keeps its gradient -- and comes back as a device tensor in the reference's (D x E') /
(D x N') shape.  A feature of another dtype (integer targets, masks) is indexed where it lives and keeps dtype and placement; reducing
one is an ArgumentError.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .graphs import GNNGraph
from .plans import _rows_index

_AGGRS = {k: _lib.AGGR[k] for k in ("+", "sum", "add", "mean", "max", "min")}
_DIRS = {"out": 0, "in": 1, "both": 2}


def _arg_error(msg):
    return _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, msg)


def _aggr_code(aggr):
    code = _AGGRS.get(aggr) if isinstance(aggr, str) else None
    if code is None:
        raise _arg_error(f"unsupported aggregation {aggr!r}; duplicate edges are combined with '+', 'mean', 'max' or 'min'")
    return code


def _device():
    if not torch.cuda.is_available():
        raise _lib.NgpdeError(_lib.ERR_HIP, "no HIP device: the graph transforms run on the GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _coo(g, dev):
    """the graph's 0-based int32 COO lists on `dev` (uploaded once per structure)"""
    coo = g._shared.get(("coo", str(dev)))
    if coo is None:
        coo = (torch.as_tensor(g._s0.astype(np.int32), device=dev), torch.as_tensor(g._t0.astype(np.int32), device=dev))
        g._shared[("coo", str(dev))] = coo
    return coo


def _is_f32(v):
    return v.dtype == (torch.float32 if isinstance(v, torch.Tensor) else np.float32)


def _f32_device(v, dev):
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    return t.to(dev, torch.float32)


def _outer(x):
    """the number of rows of a feature seen as a matrix over its last dimension (reshape(-1, n) cannot tell when n == 0)"""
    return int(np.prod(tuple(x.shape[:-1]), dtype=np.int64))


class _Index:
    """an int64 index list on the device, with its host copy made on first use (features that live on the host)"""

    def __init__(self, dev_index):
        self.dev = dev_index
        self._host = None

    def __len__(self):
        return int(self.dev.numel())

    def host(self):
        if self._host is None:
            self._host = self.dev.cpu().numpy()
        return self._host


def _select(v, index, n, dev):
    """v[..., index] for a feature whose last dimension has n entries"""
    if _is_f32(v):
        x = _f32_device(v, dev)
        rows = _rows_index(x.reshape(_outer(x), n), index.dev, n, False)     # (D x n) is [outer = D][n] with rows of one float
        return rows.reshape(tuple(x.shape[:-1]) + (len(index),))
    if isinstance(v, torch.Tensor):
        return v[..., index.dev.to(v.device)]
    return np.asarray(v)[..., index.host()]


def _select_all(data, index, n, dev):
    return {k: _select(v, index, n, dev) for k, v in data.items()}


class _Coalesced:
    """what ngpde_coo_coalesce wrote: the groups of duplicate edges of a structure"""

    def __init__(self, g, dev, symmetrize, coo=None):
        lib = _lib.load()
        s, t = _coo(g, dev) if coo is None else coo          # (coo: the lists to group in place of g's own -- editing.to_unidirected)
        e = g.num_edges
        m = 2 * e if symmetrize else e
        self.n_rows, self.copies = e, 2 if symmetrize else 1
        s_out = torch.empty(m, dtype=torch.int32, device=dev)
        t_out = torch.empty(m, dtype=torch.int32, device=dev)
        self.group_ptr = torch.empty(m + 1, dtype=torch.int32, device=dev)
        self.member = torch.empty(m, dtype=torch.int32, device=dev)
        self.group_of = torch.empty(m, dtype=torch.int32, device=dev)
        n_out = C.c_int64(0)
        _lib.check(lib.ngpde_coo_coalesce(g.num_nodes, e, _lib.ptr(s), _lib.ptr(t), 0, int(symmetrize), _lib.ptr(s_out), _lib.ptr(t_out),
                                          _lib.ptr(self.group_ptr), _lib.ptr(self.member), _lib.ptr(self.group_of), C.byref(n_out),
                                          _lib.current_stream()))
        self.n_groups = int(n_out.value)
        self.s, self.t = s_out[:self.n_groups], t_out[:self.n_groups]


class _GroupReduceFn(torch.autograd.Function):
    """x [E][d] -> [G][d]: every group of duplicate edges combined in member order"""

    @staticmethod
    def forward(ctx, x, coal, aggr):
        x = x.contiguous()
        d = x.shape[1]
        out = torch.empty((coal.n_groups, d), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().ngpde_group_reduce_forward(coal.n_groups, coal.n_rows, d, aggr, _lib.ptr(coal.group_ptr), _lib.ptr(coal.member),
                                                          _lib.ptr(x), _lib.ptr(out), _lib.current_stream()))
        ctx.coal, ctx.aggr, ctx.shape = coal, aggr, tuple(x.shape)
        if aggr in (_lib.AGGR["max"], _lib.AGGR["min"]):
            ctx.save_for_backward(x, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        coal = ctx.coal
        x, out = ctx.saved_tensors if ctx.saved_tensors else (None, None)
        dout = dout.contiguous()
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dout.device)
        _lib.check(_lib.load().ngpde_group_reduce_backward(coal.n_groups, coal.n_rows, coal.copies, ctx.shape[1], ctx.aggr,
                                                           _lib.ptr(coal.group_ptr), _lib.ptr(coal.group_of), _lib.ptr(x), _lib.ptr(out),
                                                           _lib.ptr(dout), _lib.ptr(dx), _lib.current_stream()))
        return dx, None, None


def _reduce(v, coal, aggr, n, dev):
    """a (D x E) / (E,) float32 edge feature combined over every group: (D x E') / (E',)"""
    x = _f32_device(v, dev)
    out = _GroupReduceFn.apply(x.reshape(_outer(x), n).T, coal, aggr)
    return out.T.reshape(tuple(x.shape[:-1]) + (coal.n_groups,))


class _AppendOnesFn(torch.autograd.Function):
    """w (E,) -> (E + N,): the new loops' weights are 1 (the COO lists are written by the same launch)"""

    @staticmethod
    def forward(ctx, w, g, s, t, s_out, t_out):
        w = w.contiguous()
        w_out = torch.empty(g.num_edges + g.num_nodes, dtype=torch.float32, device=w.device)
        _lib.check(_lib.load().ngpde_coo_add_self_loops(g.num_nodes, g.num_edges, _lib.ptr(s), _lib.ptr(t), 0, _lib.ptr(w), _lib.ptr(s_out),
                                                        _lib.ptr(t_out), _lib.ptr(w_out), _lib.current_stream()))
        ctx.e = g.num_edges
        return w_out

    @staticmethod
    def backward(ctx, dw):
        return dw[:ctx.e], None, None, None, None, None


def _new_graph(s, t, n, dev, *, num_graphs, indicator, ndata, edata, gdata, edge_weight, order=None):
    """a GNNGraph over device COO lists (0-based int32), as graphs._graph_from_device_coo makes them"""
    g = GNNGraph(s.cpu().numpy(), t.cpu().numpy(), num_nodes=n, index_base=0, num_graphs=num_graphs, graph_indicator=indicator,
                 ndata=ndata or None, edata=edata or None, gdata=gdata or None, edge_weight=edge_weight)
    g._shared[("coo", str(dev))] = (s, t)            # the handle builder takes the device lists as they are
    if order is not None:
        g._shared["order"] = order
    return g


def _edge_weight_of(g):
    w = g.edge_weight
    if w is not None and int(np.prod(tuple(w.shape))) != g.num_edges:
        raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                     f"DimensionMismatch: edge_weight has {int(np.prod(tuple(w.shape)))} entries for {g.num_edges} edges")
    return w


# ---- queries --------------------------------------------------------------------------------------------------------------------


def degree(g, dir="out", edge_weight=True):
    """[UPSTREAM GNNGraphs.degree(g; dir, edge_weight)] per node, the number of edges leaving it (dir="out"), entering it ("in") or both
    (out + in): an int32 device tensor of length N.  With weights -- edge_weight=True on a graph that carries `edge_weight`, or a
    tensor / array of E weights -- the float32 sum of the weights of those edges, added in COO order (bitwise equal from run to run)."""
    code = _DIRS.get(dir) if isinstance(dir, str) else None
    if code is None:
        raise _arg_error(f"dir must be 'out', 'in' or 'both', not {dir!r}")
    if edge_weight is True:
        w = _edge_weight_of(g)
    elif edge_weight is False or edge_weight is None:
        w = None
    else:
        w = edge_weight if isinstance(edge_weight, torch.Tensor) else np.asarray(edge_weight)
        if int(np.prod(tuple(w.shape))) != g.num_edges:
            raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                         f"DimensionMismatch: edge_weight has {int(np.prod(tuple(w.shape)))} entries for {g.num_edges} edges")
    dev = _device()
    s, t = _coo(g, dev)
    counts = sums = wd = None
    if w is None:
        counts = torch.empty(g.num_nodes, dtype=torch.int32, device=dev)
    else:
        wd = _f32_device(w, dev).detach().reshape(-1).contiguous()
        sums = torch.empty(g.num_nodes, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ngpde_coo_degree(g.num_nodes, g.num_edges, _lib.ptr(s), _lib.ptr(t), 0, code, _lib.ptr(wd), _lib.ptr(counts),
                                            _lib.ptr(sums), _lib.current_stream()))
    return counts if w is None else sums


def _flags(g):
    """(has_self_loops, has_multi_edges, is_bidirected) of the structure: one library call, kept with the structure"""
    f = g._shared.get("flags")
    if f is None:
        dev = _device()
        s, t = _coo(g, dev)
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.load().ngpde_coo_flags(g.num_nodes, g.num_edges, _lib.ptr(s), _lib.ptr(t), 0, C.byref(a), C.byref(b), C.byref(c),
                                               _lib.current_stream()))
        f = g._shared["flags"] = (bool(a.value), bool(b.value), bool(c.value))
    return f


def has_self_loops(g):
    """[UPSTREAM GNNGraphs.has_self_loops] true if some edge has s == t"""
    return _flags(g)[0]


def has_multi_edges(g):
    """[UPSTREAM GNNGraphs.has_multi_edges] true if some (s, t) pair occurs twice"""
    return _flags(g)[1]


def is_bidirected(g):
    """[UPSTREAM GNNGraphs.is_bidirected] true if every pair (s, t) occurs as often as (t, s)"""
    return _flags(g)[2]


# ---- transforms -----------------------------------------------------------------------------------------------------------------


def add_self_loops(g):
    """[UPSTREAM GNNGraphs.add_self_loops] the E edges of g in order, then (i, i) for every node i; existing loops are not looked for.
    `edge_weight`, if present, gets N ones appended.  A graph with edge features is refused, as upstream asserts."""
    if g.edata:
        raise _arg_error("add_self_loops: the graph carries edge features (edata); the new loops would have none")
    w = _edge_weight_of(g)
    dev = _device()
    s, t = _coo(g, dev)
    m = g.num_edges + g.num_nodes
    s_out = torch.empty(m, dtype=torch.int32, device=dev)
    t_out = torch.empty(m, dtype=torch.int32, device=dev)
    if w is not None:
        w = _AppendOnesFn.apply(_f32_device(w, dev).reshape(-1), g, s, t, s_out, t_out)
    else:
        _lib.check(_lib.load().ngpde_coo_add_self_loops(g.num_nodes, g.num_edges, _lib.ptr(s), _lib.ptr(t), 0, None, _lib.ptr(s_out),
                                                        _lib.ptr(t_out), None, _lib.current_stream()))
    return _new_graph(s_out, t_out, g.num_nodes, dev, num_graphs=g.num_graphs, indicator=g.graph_indicator, ndata=g.ndata, edata=None,
                      gdata=g.gdata, edge_weight=w, order=g._shared.get("order"))


def _compact(g, dev, nodes, drop_self_loops):
    """ngpde_coo_compact: (s', t', the kept COO positions as an _Index)"""
    s, t = _coo(g, dev)
    e = g.num_edges
    s_out = torch.empty(e, dtype=torch.int32, device=dev)
    t_out = torch.empty(e, dtype=torch.int32, device=dev)
    kept = torch.empty(e, dtype=torch.int64, device=dev)
    n_out = C.c_int64(0)
    _lib.check(_lib.load().ngpde_coo_compact(g.num_nodes, e, _lib.ptr(s), _lib.ptr(t), 0, 0 if nodes is None else int(nodes.numel()),
                                             _lib.ptr(nodes), int(drop_self_loops), _lib.ptr(s_out), _lib.ptr(t_out), _lib.ptr(kept),
                                             C.byref(n_out), _lib.current_stream()))
    k = int(n_out.value)
    return s_out[:k], t_out[:k], _Index(kept[:k])


def remove_self_loops(g):
    """[UPSTREAM GNNGraphs.remove_self_loops] the edges with s != t, in COO order; `edge_weight` and every edge feature follow them"""
    w = _edge_weight_of(g)
    dev = _device()
    s, t, kept = _compact(g, dev, None, True)
    return _new_graph(s, t, g.num_nodes, dev, num_graphs=g.num_graphs, indicator=g.graph_indicator, ndata=g.ndata,
                      edata=_select_all(g.edata, kept, g.num_edges, dev), gdata=g.gdata,
                      edge_weight=None if w is None else _select(w, kept, g.num_edges, dev).reshape(-1), order=g._shared.get("order"))


def _coalesce(g, aggr, symmetrize, what, coo=None):
    code = _aggr_code(aggr)
    w = _edge_weight_of(g)
    for k, v in list(g.edata.items()) + ([("edge_weight", w)] if w is not None else []):
        if not _is_f32(v):
            raise _arg_error(f"{what}: edge feature '{k}' is {v.dtype}, only float32 features can be combined over duplicate edges")
    dev = _device()
    coal = _Coalesced(g, dev, symmetrize, coo and coo(dev))
    edata = {k: _reduce(v, coal, code, g.num_edges, dev) for k, v in g.edata.items()}
    return _new_graph(coal.s, coal.t, g.num_nodes, dev, num_graphs=g.num_graphs, indicator=g.graph_indicator, ndata=g.ndata, edata=edata,
                      gdata=g.gdata, edge_weight=None if w is None else _reduce(w, coal, code, g.num_edges, dev).reshape(-1),
                      order=g._shared.get("order"))


def remove_multi_edges(g, aggr="+"):
    """[UPSTREAM GNNGraphs.remove_multi_edges(g; aggr)] one edge per distinct (s, t), ordered by source, then target (upstream sorts the
    code (s-1)*n + t).  `edge_weight` and every edge feature are combined over each group of duplicates with aggr -- "+", "mean", "max"
    or "min" -- the members taken in ascending COO position."""
    return _coalesce(g, aggr, False, "remove_multi_edges")


def to_bidirected(g):
    """[UPSTREAM GNNGraphs.to_bidirected] the edges [s; t], [t; s] coalesced as remove_multi_edges does, with aggr="mean": every pair
    ends up in both directions, once.  Features and weights are those of the list concatenated with itself (a self loop's group holds
    both of its copies); the 2E-edge list is never made."""
    return _coalesce(g, "mean", True, "to_bidirected")


def _node_index(nodes, dev):
    if isinstance(nodes, torch.Tensor):
        t = nodes.reshape(-1).to(dev, torch.int64)
    else:
        t = torch.as_tensor(np.asarray(nodes, dtype=np.int64).reshape(-1), device=dev)
    return _Index(t.contiguous())


def _induced(g, nodes, dev):
    """the subgraph on `nodes` (an _Index): edges, node and edge features; the caller adds what is per graph"""
    w = _edge_weight_of(g)
    s, t, kept = _compact(g, dev, nodes.dev, False)
    return dict(s=s, t=t, n=len(nodes), dev=dev, ndata=_select_all(g.ndata, nodes, g.num_nodes, dev),
                edata=_select_all(g.edata, kept, g.num_edges, dev),
                edge_weight=None if w is None else _select(w, kept, g.num_edges, dev).reshape(-1))


def induced_subgraph(g, nodes):
    """[UPSTREAM GNNGraphs.induced_subgraph(g, nodes)] the graph on the listed nodes (distinct, 0-based): node k of the result is
    nodes[k], an edge is kept iff both its ends are, kept edges stay in COO order.  Node and edge features follow; graph features and
    the number of graphs are kept.  A node out of range or listed twice is an ArgumentError."""
    dev = _device()
    nodes = _node_index(nodes, dev)
    p = _induced(g, nodes, dev)
    gi = None if g.graph_indicator is None else g.graph_indicator[nodes.host()]
    return _new_graph(p.pop("s"), p.pop("t"), p.pop("n"), p.pop("dev"), num_graphs=g.num_graphs, indicator=gi, gdata=g.gdata, **p)


def _graph_positions(g, i):
    """`i` of getgraph as a list of graph positions, checked on the host"""
    single = isinstance(i, (int, np.integer)) and not isinstance(i, bool)
    try:
        ids = [int(i)] if single else [int(k) for k in i]
        exact = single or all(int(k) == k for k in i)
    except (TypeError, ValueError):
        ids, exact = [], False
    if not exact or not ids:
        raise _arg_error(f"getgraph: i must be a graph position or a non-empty list of them, not {i!r}")
    if min(ids) < 0 or max(ids) >= g.num_graphs:
        raise _arg_error(f"getgraph: graph position outside 0:{g.num_graphs - 1} in {ids}")
    if any(b <= a for a, b in zip(ids, ids[1:])):
        raise _arg_error(f"getgraph: the graph positions must be strictly increasing, not {ids}")
    if g.num_graphs > 1 and g.graph_indicator is None:
        raise _arg_error(f"getgraph: the graph holds {g.num_graphs} graphs but no graph_indicator: build it with batch(), radius_graph / "
                         "knn_graph(..., graph_indicator=) or GNNGraph(..., graph_indicator=)")
    return ids


def getgraph(g, i, nmap=False):
    """[UPSTREAM GNNGraphs.getgraph(g, i; nmap)] the member(s) `i` of a batch: `i` is a graph position (0-based) or a strictly increasing
    list of them.  The nodes whose graph is in `i`, in ascending node order, with the edges among them (induced_subgraph's primitive);
    the new graph ids are the positions within `i`, the graph features the columns `i`.  nmap=True also returns the int64 device tensor
    of the kept nodes' ids in g."""
    ids = _graph_positions(g, i)
    dev = _device()
    if g.graph_indicator is None:
        node_ids, indicator = np.arange(g.num_nodes, dtype=np.int64), None
    else:
        position = np.full(g.num_graphs, -1, dtype=np.int64)
        position[ids] = np.arange(len(ids))
        new_id = position[g.graph_indicator]
        node_ids = np.flatnonzero(new_id >= 0).astype(np.int64)
        indicator = new_id[node_ids] if len(ids) > 1 else None
    nodes = _node_index(node_ids, dev)
    nodes._host = node_ids
    p = _induced(g, nodes, dev)
    gdata = g.gdata
    if gdata and g.num_graphs > 1:
        gdata = _select_all(gdata, _node_index(ids, dev), g.num_graphs, dev)
    out = _new_graph(p.pop("s"), p.pop("t"), p.pop("n"), p.pop("dev"), num_graphs=len(ids), indicator=indicator, gdata=gdata, **p)
    return (out, nodes.dev) if nmap else out


def unbatch(g):
    """[UPSTREAM MLUtils.unbatch(::GNNGraph)] the members of a batch: the inverse of batch(), features included"""
    return [getgraph(g, i) for i in range(g.num_graphs)]
