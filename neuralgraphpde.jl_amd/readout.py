"""The per-graph readouts the reference re-exports from GraphNeuralNetworks.jl (/root/reference/src/NeuralGraphPDE.jl:5-7):
`reduce_nodes`, `reduce_edges`, `softmax_nodes`, `softmax_edges`, `broadcast_nodes`, `broadcast_edges` -- one column per graph of a
batch (`batch()`, `radius_graph(..., graph_indicator=)`) out of its nodes' or edges' columns, and back:

    uT, _ = node(u0, ps, st)                       # (D x N) over a batch of clouds
    loss = (reduce_nodes("mean", g, uT) * R).sum() # (D x num_graphs)

Conventions as in msgpass.py: node arrays are (D x N), edge arrays (D x E) in the graph's COO order (a vector of E entries is one
row), per-graph arrays (D x num_graphs); `aggr` is "+", "mean", "max" or "min" (their other spellings in _lib.AGGR included); an
empty graph gives 0 for + and mean, -inf / +inf for max / min.  An edge belongs to the graph of its source.

Every function is a torch.autograd.Function over the library's readout entries (include/ngpde.h, "the per-graph readouts"):
atomic-free, bitwise reproducible, capturable into a HIP graph.  The plan of a structure -- its items cut into fixed chunks -- is
built once per device and shared by every copy of the graph.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import functional as F
from .layers import rows_of
from .msgpass import _edge_rows, _node_rows

_AGGRS = (_lib.AGGR["+"], _lib.AGGR["mean"], _lib.AGGR["max"], _lib.AGGR["min"])


def _aggr_code(aggr):
    code = _lib.AGGR.get(aggr) if isinstance(aggr, str) else None
    if code not in _AGGRS:
        raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT,
                                 f"unsupported aggregation {aggr!r}; the readouts take '+', 'mean', 'max' and 'min'")
    return code


def _indicator0(g):
    """0-based int32 graph id per node, or None for a single graph"""
    if g.num_graphs == 1:
        return None
    if g.graph_indicator is None:
        raise _lib.ArgumentError(
            _lib.ERR_INVALID_ARGUMENT,
            f"the graph holds {g.num_graphs} graphs but no graph_indicator: build it with batch(), radius_graph / knn_graph(..., "
            "graph_indicator=) or GNNGraph(..., graph_indicator=) (the padded batch of batches.py is such a graph: read out its "
            "members before padding)")
    return g.graph_indicator


def graph_indicator(g, edges=False):
    """[UPSTREAM GNNGraphs.graph_indicator(g; edges)] the 1-based graph id of every node, or with edges=True of every edge's source
    in COO order; all ones for a single graph"""
    gi = _indicator0(g)
    if gi is None:
        return np.ones(g.num_edges if edges else g.num_nodes, dtype=np.int32)
    return (gi[g._s0] if edges else gi) + np.int32(1)


class _Plan:
    """owner of one ngpde_readout_t: the nodes or the edges of a structure cut into chunks by graph"""

    def __init__(self, g, kind, dev):
        lib = _lib.load()
        _lib.flush_destroy()
        self.ptr = None
        gi = _indicator0(g)
        ids = index = None
        if gi is not None:
            ids = torch.as_tensor(gi, device=dev)
            if kind == "edges":
                coo = g._shared.get(("coo", str(dev)))
                if coo is None:
                    coo = (torch.as_tensor(g._s0.astype(np.int32), device=dev), torch.as_tensor(g._t0.astype(np.int32), device=dev))
                    g._shared[("coo", str(dev))] = coo
                index = coo[0]
        self.n_items = g.num_nodes if kind == "nodes" else g.num_edges
        self.n_segments = g.num_graphs
        out = C.c_void_p()
        _lib.check(lib.ngpde_readout_create(self.n_items, _lib.ptr(ids), _lib.ptr(index), 0, self.n_segments, _lib.current_stream(),
                                            C.byref(out)))
        self.ptr = out

    def info(self):
        n, s, c, k, r = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        _lib.check(_lib.load().ngpde_readout_info(self.ptr, C.byref(n), C.byref(s), C.byref(c), C.byref(k), C.byref(r)))
        return dict(n_items=n.value, n_segments=s.value, contiguous=bool(c.value), n_chunks=k.value, chunk_rows=r.value)

    def workspace(self, d, device):
        return F._ws(_lib.load().ngpde_readout_workspace_bytes(self.ptr, d), device)

    def __del__(self):
        try:
            if self.ptr:
                _lib.destroy_later("ngpde_readout_destroy", self.ptr)     # (not inside a HIP-graph capture: see _lib.destroy_later)
                self.ptr = None
        except Exception:
            pass


def _plan(g, kind, device):
    """the structure's plan on `device`, shared by every copy of the graph"""
    _indicator0(g)      # (a batch that does not know its nodes' graphs is refused before anything else)
    if device.type != "cuda":
        raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT,
                                 "the readouts run on the MI355X only: move the array to the GPU (there is no CPU fallback)")
    dev = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
    key = ("readout", kind, str(dev))
    p = g._shared.get(key)
    if p is None or p.n_segments != g.num_graphs:
        p = g._shared[key] = _Plan(g, kind, dev)
    return p


# ---- autograd nodes over the C ABI --------------------------------------------------------------------------------------------


class _ReduceFn(torch.autograd.Function):
    """x [n][d] -> [S][d]"""

    @staticmethod
    def forward(ctx, x, plan, aggr):
        lib = _lib.load()
        x = x.contiguous()
        d = x.shape[1]
        out = torch.empty((plan.n_segments, d), dtype=torch.float32, device=x.device)
        ws = plan.workspace(d, x.device)
        _lib.check(lib.ngpde_readout_reduce_forward(plan.ptr, d, aggr, _lib.ptr(x), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                                    _lib.current_stream()))
        ctx.plan, ctx.aggr, ctx.shape = plan, aggr, tuple(x.shape)
        if aggr in (_lib.AGGR["max"], _lib.AGGR["min"]):
            ctx.save_for_backward(x, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, out = ctx.saved_tensors if ctx.saved_tensors else (None, None)
        dout = dout.contiguous()
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dout.device)
        _lib.check(lib.ngpde_readout_reduce_backward(ctx.plan.ptr, ctx.shape[1], ctx.aggr, _lib.ptr(x), _lib.ptr(out), _lib.ptr(dout),
                                                     _lib.ptr(dx), _lib.current_stream()))
        return dx, None, None


class _SoftmaxFn(torch.autograd.Function):
    """x [n][d] -> y [n][d]"""

    @staticmethod
    def forward(ctx, x, plan):
        lib = _lib.load()
        x = x.contiguous()
        d = x.shape[1]
        y = torch.empty_like(x)
        ws = plan.workspace(d, x.device)
        _lib.check(lib.ngpde_readout_softmax_forward(plan.ptr, d, _lib.ptr(x), _lib.ptr(y), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
        ctx.plan = plan
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        d = y.shape[1]
        dx = torch.empty_like(y)
        ws = ctx.plan.workspace(d, y.device)
        _lib.check(lib.ngpde_readout_softmax_backward(ctx.plan.ptr, d, _lib.ptr(y), _lib.ptr(dy), _lib.ptr(dx), _lib.ptr(ws), ws.numel(),
                                                      _lib.current_stream()))
        return dx, None


class _BroadcastFn(torch.autograd.Function):
    """u [S][d] -> [n][d]"""

    @staticmethod
    def forward(ctx, u, plan):
        lib = _lib.load()
        u = u.contiguous()
        d = u.shape[1]
        out = torch.empty((plan.n_items, d), dtype=torch.float32, device=u.device)
        _lib.check(lib.ngpde_readout_broadcast_forward(plan.ptr, d, _lib.ptr(u), _lib.ptr(out), _lib.current_stream()))
        ctx.plan, ctx.d = plan, d
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        dout = dout.contiguous()
        du = torch.empty((ctx.plan.n_segments, ctx.d), dtype=torch.float32, device=dout.device)
        ws = ctx.plan.workspace(ctx.d, dout.device)
        _lib.check(lib.ngpde_readout_broadcast_backward(ctx.plan.ptr, ctx.d, _lib.ptr(dout), _lib.ptr(du), _lib.ptr(ws), ws.numel(),
                                                        _lib.current_stream()))
        return du, None


def _graph_rows(u, g):
    ur = rows_of(u)
    if ur.shape[0] != g.num_graphs:
        raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                     f"DimensionMismatch: u has {ur.shape[0]} columns, graph has {g.num_graphs} graphs")
    return ur


# ---- public API -------------------------------------------------------------------------------------------------------------


def reduce_nodes(aggr, g, x):
    """out[:, k] = aggr over the nodes of graph k of x[:, i]; x (D x N) -> (D x num_graphs)"""
    code = _aggr_code(aggr)
    xr = _node_rows(x, g, "x")
    return _ReduceFn.apply(xr, _plan(g, "nodes", xr.device), code).T


def reduce_edges(aggr, g, e):
    """out[:, k] = aggr over the edges of graph k of e[:, j]; e (D x E) or (E,) in COO order -> (D x num_graphs)"""
    code = _aggr_code(aggr)
    er = _edge_rows(e, g)
    return _ReduceFn.apply(er, _plan(g, "edges", er.device), code).T


def softmax_nodes(g, x):
    """per graph and row, the softmax of x over the graph's nodes; x (D x N) -> (D x N)"""
    xr = _node_rows(x, g, "x")
    return _SoftmaxFn.apply(xr, _plan(g, "nodes", xr.device)).T


def softmax_edges(g, e):
    """per graph and row, the softmax of e over the graph's edges; e (D x E) or (E,) in COO order -> the same shape"""
    if not isinstance(e, torch.Tensor):
        e = torch.as_tensor(e)
    er = _edge_rows(e, g)
    y = _SoftmaxFn.apply(er, _plan(g, "edges", er.device)).T
    return y.reshape(-1) if e.dim() == 1 else y


def broadcast_nodes(g, u):
    """out[:, i] = u[:, graph of node i]; u (D x num_graphs) -> (D x N)"""
    ur = _graph_rows(u, g)
    return _BroadcastFn.apply(ur, _plan(g, "nodes", ur.device)).T


def broadcast_edges(g, u):
    """out[:, j] = u[:, graph of edge j]; u (D x num_graphs) -> (D x E) in COO order"""
    ur = _graph_rows(u, g)
    return _BroadcastFn.apply(ur, _plan(g, "edges", ur.device)).T
