"""The message-passing API the reference re-exports from GraphNeuralNetworks.jl (/root/reference/src/NeuralGraphPDE.jl:5-11):
`propagate`, `apply_edges`, `aggregate_neighbors`, `softmax_edge_neighbors` and the built-in messages `copy_xj`, `copy_xi`,
`xi_dot_xj`, `e_mul_xj`, `w_mul_xj` -- what a user layer is written around (docs/src/devdoc.md:47-52):

    def message(xi, xj, e):
        return dense(torch.cat([xi["h"], xj["h"], xj["x"] - xi["x"]]), ps, st)[0]
    y = propagate(message, g, "mean", xi=xs, xj=xs)

Node arrays are (D x N) and edge arrays (D x E), as everywhere in the package; edge arrays a caller passes in or gets back are in
the graph's COO order (g.edata order).  `xi` / `xj` may be a tensor, a dict (NamedTuple) of tensors or None; `e` a tensor, a dict
or None.  `aggr` is one of the names in _lib.AGGR; an empty neighbourhood gives 0 for + and mean, -inf / +inf for max / min and 1
for *.

Every step is a library launch (include/ngpde.h, "the public message-passing API"): the gathers, the fused built-ins
(propagate(e_mul_xj | w_mul_xj | copy_xj, g, + | mean), apply_edges(xi_dot_xj)), the edge softmax, the permutations between COO
order and the library's edge order, and the segmented reductions, each with its pullback as a torch.autograd.Function.

A user message function is called ONCE on the whole edge set, with the gathered arrays as (D x E) views whose columns are the
edges in the library's order (grouped by target), not COO order: like every message of the reference, it must treat each edge
column on its own.
"""
from __future__ import annotations

import torch

from . import _lib
from . import functional as F
from .layers import rows_of

_MAX_GATHER = 4     # arrays per ngpde_gather_forward launch


# ---- built-in messages [GraphNeuralNetworks.jl], also usable as plain functions of (D x E) arrays -------------------------------


def _ecol(e):
    return e.reshape(1, -1) if e.dim() == 1 else e


def copy_xj(xi, xj, e):
    return xj


def copy_xi(xi, xj, e):
    return xi


def xi_dot_xj(xi, xj, e):
    return (xi * xj).sum(dim=0, keepdim=True)


def e_mul_xj(xi, xj, e):
    return _ecol(e) * xj


def w_mul_xj(xi, xj, w):
    """xj scaled by the edge weights; propagate / apply_edges pass the graph's weights (ones where it has none) as `w`"""
    return _ecol(w) * xj


# ---- autograd nodes over the C ABI --------------------------------------------------------------------------------------------


def _aggr_code(aggr):
    code = _lib.AGGR.get(aggr) if isinstance(aggr, str) else None
    if code is None:
        raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, f"unsupported aggregation {aggr!r}; one of {list(_lib.AGGR)}")
    return code


class _GatherFn(torch.autograd.Function):
    """xi_p = X[t_p], xj_p = X[s_p] ([E][w], p order) for up to 4 arrays in one launch; `sides`: per array (want xi, want xj).
    The outputs are the wanted gathers in array order, xi before xj."""

    @staticmethod
    def forward(ctx, handle, n_edges, sides, *xs):
        lib = _lib.load()
        F._need_cuda(*xs)
        xs = [x.contiguous() for x in xs]
        outs_i = [torch.empty((n_edges, x.shape[1]), dtype=torch.float32, device=x.device) if wi else None for x, (wi, _) in zip(xs, sides)]
        outs_j = [torch.empty((n_edges, x.shape[1]), dtype=torch.float32, device=x.device) if wj else None for x, (_, wj) in zip(xs, sides)]
        _lib.check(lib.ngpde_gather_forward(handle.ptr, len(xs), F._ptr_array(xs), F._int_array([x.shape[1] for x in xs]),
                                            F._ptr_array(outs_i), F._ptr_array(outs_j), _lib.current_stream()))
        ctx.handle, ctx.sides = handle, sides
        ctx.shapes = [tuple(x.shape) for x in xs]
        ctx.set_materialize_grads(False)
        out = []
        for oi, oj in zip(outs_i, outs_j):
            out += [o for o in (oi, oj) if o is not None]
        return tuple(out)

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib.load()
        it = iter(grads)
        gi, gj = [], []
        for wi, wj in ctx.sides:
            gi.append(next(it) if wi else None)
            gj.append(next(it) if wj else None)
        gi = [None if g is None else g.contiguous() for g in gi]
        gj = [None if g is None else g.contiguous() for g in gj]
        if all(g is None for g in gi + gj):
            return (None, None, None, *[None] * len(ctx.shapes))
        dev = next(g for g in gi + gj if g is not None).device
        dxs = [torch.empty(s, dtype=torch.float32, device=dev) if ctx.needs_input_grad[3 + k] else None for k, s in enumerate(ctx.shapes)]
        _lib.check(lib.ngpde_gather_backward(ctx.handle.ptr, len(dxs), F._int_array([s[1] for s in ctx.shapes]), F._ptr_array(gi),
                                             F._ptr_array(gj), F._ptr_array(dxs), _lib.current_stream()))
        return (None, None, None, *dxs)


class _EmulFn(torch.autograd.Function):
    """propagate(e_mul_xj | w_mul_xj | copy_xj, g, + | mean): x [N][d], e [E][1 or d] COO order or None -> [N][d]"""

    @staticmethod
    def forward(ctx, x, e, handle, aggr):
        lib = _lib.load()
        F._need_cuda(x, e)
        x = x.contiguous()
        e = None if e is None else e.contiguous()
        ew = 0 if e is None else e.shape[1]
        out = torch.empty_like(x)
        _lib.check(lib.ngpde_propagate_emul_forward(handle.ptr, x.shape[1], ew, aggr, _lib.ptr(x), _lib.ptr(e), _lib.ptr(out),
                                                    _lib.current_stream()))
        ctx.handle, ctx.aggr, ctx.ew = handle, aggr, ew
        ctx.save_for_backward(x, e)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, e = ctx.saved_tensors
        dout = dout.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        de = torch.empty_like(e) if (e is not None and ctx.needs_input_grad[1]) else None
        _lib.check(lib.ngpde_propagate_emul_backward(ctx.handle.ptr, x.shape[1], ctx.ew, ctx.aggr, _lib.ptr(x), _lib.ptr(e), _lib.ptr(dout),
                                                     _lib.ptr(dx), _lib.ptr(de), _lib.current_stream()))
        return dx, de, None, None


class _DotFn(torch.autograd.Function):
    """apply_edges(xi_dot_xj): xi, xj [N][d] -> [E][1] in COO order"""

    @staticmethod
    def forward(ctx, xi, xj, handle, n_edges):
        lib = _lib.load()
        F._need_cuda(xi, xj)
        xi, xj = xi.contiguous(), xj.contiguous()
        out = torch.empty((n_edges, 1), dtype=torch.float32, device=xi.device)
        _lib.check(lib.ngpde_apply_edges_dot_forward(handle.ptr, xi.shape[1], _lib.ptr(xi), _lib.ptr(xj), _lib.ptr(out), _lib.current_stream()))
        ctx.handle = handle
        ctx.save_for_backward(xi, xj)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        xi, xj = ctx.saved_tensors
        dout = dout.contiguous()
        dxi = torch.empty_like(xi) if ctx.needs_input_grad[0] else None
        dxj = torch.empty_like(xj) if ctx.needs_input_grad[1] else None
        _lib.check(lib.ngpde_apply_edges_dot_backward(ctx.handle.ptr, xi.shape[1], _lib.ptr(xi), _lib.ptr(xj), _lib.ptr(dout), _lib.ptr(dxi),
                                                      _lib.ptr(dxj), _lib.current_stream()))
        return dxi, dxj, None, None


class _SoftmaxFn(torch.autograd.Function):
    """softmax_edge_neighbors: e [E][H] COO order -> y [E][H] COO order"""

    @staticmethod
    def forward(ctx, e, handle):
        lib = _lib.load()
        F._need_cuda(e)
        e = F._f32(e)                # (softmax_edge_*_kernel read one float at a time)
        y = torch.empty_like(e)
        _lib.check(lib.ngpde_softmax_edge_neighbors_forward(handle.ptr, e.shape[1], _lib.ptr(e), _lib.ptr(y), _lib.current_stream()))
        ctx.handle = handle
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (y,) = ctx.saved_tensors
        dy = F._f32(dy)
        de = torch.empty_like(y)
        _lib.check(lib.ngpde_softmax_edge_neighbors_backward(ctx.handle.ptr, y.shape[1], _lib.ptr(y), _lib.ptr(dy), _lib.ptr(de),
                                                             _lib.current_stream()))
        return de, None


class _SegmentReduceFn(torch.autograd.Function):
    """aggregate_neighbors on p-order rows: m [E][d] -> [N][d] (ngpde_segment_reduce_*)"""

    @staticmethod
    def forward(ctx, m, handle, aggr, n_nodes):
        lib = _lib.load()
        F._need_cuda(m)
        m = m.contiguous()
        out = torch.empty((n_nodes, m.shape[1]), dtype=torch.float32, device=m.device)
        _lib.check(lib.ngpde_segment_reduce_forward(handle.ptr, m.shape[1], aggr, _lib.ptr(m), _lib.ptr(out), _lib.current_stream()))
        ctx.handle, ctx.aggr = handle, aggr
        ctx.save_for_backward(m, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        m, out = ctx.saved_tensors
        dout = dout.contiguous()
        dm = torch.empty_like(m)
        _lib.check(lib.ngpde_segment_reduce_backward(ctx.handle.ptr, m.shape[1], ctx.aggr, _lib.ptr(m), _lib.ptr(out), _lib.ptr(dout),
                                                     _lib.ptr(dm), _lib.current_stream()))
        return dm, None, None, None


# ---- argument plumbing ----------------------------------------------------------------------------------------------------------


def _node_rows(x, g, what):
    xr = rows_of(x)
    if xr.shape[0] != g.num_nodes:
        raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                     f"DimensionMismatch: {what} has {xr.shape[0]} columns, graph has {g.num_nodes} nodes")
    return xr


def _edge_rows(e, g, what="e"):
    """(w x E) or (E,) edge array -> [E][w] float32 rows"""
    if not isinstance(e, torch.Tensor):
        e = torch.as_tensor(e)
    er = rows_of(_ecol(e))
    if er.shape[0] != g.num_edges:
        raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                     f"DimensionMismatch: {what} has {er.shape[0]} columns, graph has {g.num_edges} edges")
    return er


def _edge_weight_rows(g, device):
    """[E][1] of the graph's edge weights, or ones"""
    w = g.edge_weight
    if w is None:
        return torch.ones((g.num_edges, 1), dtype=torch.float32, device=device)
    w = w if isinstance(w, torch.Tensor) else torch.as_tensor(w)
    return _edge_rows(w.detach().to(device, torch.float32).reshape(-1), g, "edge_weight")


def _gather(g, handle, xi, xj):
    """the gathered (D x E) views (p order) of xi at the targets and xj at the sources, tensors or dicts as given; an array passed on
    both sides is read once and gets one gradient"""
    arrays, sides = [], []          # unique tensors (by identity) and their (at target, at source) wants
    index = {}

    def add(t, side):
        k = id(t)
        if k not in index:
            index[k] = len(arrays)
            arrays.append(t)
            sides.append([False, False])
        sides[index[k]][side] = True
        return index[k]

    def slots(x, side, what):
        if x is None:
            return None
        if isinstance(x, dict):
            return {k: add(v, side) for k, v in x.items()}
        return add(x, side)

    si, sj = slots(xi, 0, "xi"), slots(xj, 1, "xj")
    rows = [_node_rows(t, g, "a node array") for t in arrays]
    got_i, got_j = [None] * len(rows), [None] * len(rows)
    for k0 in range(0, len(rows), _MAX_GATHER):
        part = list(range(k0, min(k0 + _MAX_GATHER, len(rows))))
        outs = _GatherFn.apply(handle, g.num_edges, tuple(tuple(sides[k]) for k in part), *[rows[k] for k in part])
        outs = iter((outs,) if isinstance(outs, torch.Tensor) else outs)
        for k in part:
            if sides[k][0]:
                got_i[k] = next(outs)
            if sides[k][1]:
                got_j[k] = next(outs)

    def views(s, got):
        if s is None:
            return None
        if isinstance(s, dict):
            return {k: got[v].T for k, v in s.items()}
        return got[s].T

    return views(si, got_i), views(sj, got_j)


def _permuted(e, g, handle):
    """e (COO order, tensor or dict) -> (w x E) views in p order"""
    if e is None:
        return None
    if isinstance(e, dict):
        return {k: _permuted(v, g, handle) for k, v in e.items()}
    return F.edge_permute(_edge_rows(e, g), handle).T


def _device_of(*xs):
    for x in xs:
        if isinstance(x, dict):
            d = _device_of(*x.values())
            if d is not None:
                return d
        elif isinstance(x, torch.Tensor):
            return x.device
    return None


def _edges_in_p_order(f, g, handle, xi, xj, e):
    """f(xi, xj, e) on the gathered arrays: its result as [E][D] rows in p order"""
    if f is w_mul_xj:
        dev = _device_of(xj, xi, e)
        e = F.edge_permute(_edge_weight_rows(g, dev), handle).T
    else:
        e = _permuted(e, g, handle)
    gi, gj = _gather(g, handle, xi, xj)
    m = f(gi, gj, e)
    if not isinstance(m, torch.Tensor):
        raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, f"the message function must return a (D x E) array, got {type(m).__name__}")
    mr = rows_of(_ecol(m))
    if mr.shape[0] != g.num_edges:
        raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                     f"DimensionMismatch: the message has {mr.shape[0]} columns, graph has {g.num_edges} edges")
    return mr


# ---- public API -------------------------------------------------------------------------------------------------------------


def aggregate_neighbors(g, aggr, m):
    """out[:, i] = aggr over the incoming edges of i of m[:, e]; m (D x E) in COO order -> (D x N)"""
    code = _aggr_code(aggr)
    h = g.handle()
    mp = F.edge_permute(_edge_rows(m, g, "m"), h)
    return _SegmentReduceFn.apply(mp, h, code, g.num_nodes).T


def propagate(f, g, aggr, *, xi=None, xj=None, e=None):
    """aggregate_neighbors(g, aggr, apply_edges(f, g; xi, xj, e)) -> (D x N).

    propagate(e_mul_xj | w_mul_xj | copy_xj, g, + | mean; xj=tensor) is one fused launch that writes no per-edge array; any other
    f runs on the gathered arrays (see the module docstring: f sees the edges in the library's order and must treat each edge column
    on its own) and its result is reduced by target."""
    code = _aggr_code(aggr)
    h = g.handle()
    if f in (e_mul_xj, w_mul_xj, copy_xj) and code in (_lib.AGGR["+"], _lib.AGGR["mean"]) and isinstance(xj, torch.Tensor):
        x = _node_rows(xj, g, "xj")
        if f is copy_xj:
            er = None
        elif f is w_mul_xj:
            er = _edge_weight_rows(g, x.device) if g.edge_weight is not None else None    # (no weights: w = 1, copy_xj)
        else:
            if e is None:
                raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, "e_mul_xj needs an edge array e")
            er = _edge_rows(e, g)
            if er.shape[1] not in (1, x.shape[1]):
                raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                             f"DimensionMismatch: e has {er.shape[1]} rows, xj has {x.shape[1]}; expected 1 or {x.shape[1]}")
        return _EmulFn.apply(x, er, h, code).T
    if f is xi_dot_xj and isinstance(xi, torch.Tensor) and isinstance(xj, torch.Tensor):
        # the dot products from the apply_edges launch: equal edges get bitwise-equal messages, so max / min route the gradient to
        # every one of them, as the reference's scatter pullback does
        mr = F.edge_permute(rows_of(apply_edges(xi_dot_xj, g, xi=xi, xj=xj)), h)
    else:
        mr = _edges_in_p_order(f, g, h, xi, xj, e)
    return _SegmentReduceFn.apply(mr, h, code, g.num_nodes).T


def apply_edges(f, g, *, xi=None, xj=None, e=None):
    """f(xi gathered at the targets, xj at the sources, e) -> (D x E) in COO order.  apply_edges(xi_dot_xj; xi=tensor, xj=tensor)
    is one launch that writes the result straight into COO order."""
    h = g.handle()
    if f is xi_dot_xj and isinstance(xi, torch.Tensor) and isinstance(xj, torch.Tensor):
        a, b = _node_rows(xi, g, "xi"), _node_rows(xj, g, "xj")
        if a.shape[1] != b.shape[1]:
            raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, f"DimensionMismatch: xi has {a.shape[1]} rows, xj has {b.shape[1]}")
        return _DotFn.apply(a, b, h, g.num_edges).T
    mr = _edges_in_p_order(f, g, h, xi, xj, e)
    return F.edge_permute(mr, h, inverse=True).T


def softmax_edge_neighbors(g, e):
    """per target, the softmax of e over its incoming edges; e (H x E) or (E,) in COO order -> the same shape, COO order"""
    er = _edge_rows(e, g)
    y = _SoftmaxFn.apply(er, g.handle()).T
    return y.reshape(-1) if (isinstance(e, torch.Tensor) and e.dim() == 1) else y
