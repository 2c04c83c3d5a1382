"""The graph as a matrix: the part of GNNGraphs the reference re-exports (src/NeuralGraphPDE.jl:4) that turns a graph into an operator --
`adjacency_matrix`, `laplacian_matrix`, `normalized_laplacian`, `scaled_laplacian`, `laplacian_lambda_max`, `khop_adj` and
`has_isolated_nodes`:

    L = laplacian_matrix(g)                         # the discrete diffusion operator: u' = -L u is  lambda u: -L.matmul(u)
    lam = laplacian_lambda_max(g)                   # explicit steps of u' = -Lhat u are stable for dt < 2 / lam
    T1 = scaled_laplacian(g, lambda_max=lam)        # 2 / lam * Lhat - I, the operator of Chebyshev filters: T1.matmul(X)
    g2 = khop_adj(g, 2).as_graph()                  # the graph of 2-hop neighbourhoods

A result is a `GraphMatrix`: a coalesced sparse N x N float32 matrix on the device, entries sorted by row, then column.  Positions are
0-based; `dir` is "out" (an edge s -> t is the entry (s, t)) or "in" (the transpose).  Everything runs on the device over the int32 COO
lists (include/ngpde.h, "graph matrices"; csrc/graph_matrix.hip); there is no CPU fallback, no torch sparse tensor and no hipSPARSE
call.  The values of the four assembled matrices carry the gradient to a float32 `edge_weight` that requires grad.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .graphops import _arg_error, _coo, _device, _edge_weight_of, _f32_device, _new_graph, degree
from .msgpass import e_mul_xj, propagate

ADJ, LAPLACIAN, NORM_LAPLACIAN = 0, 1, 2          # NGPDE_MATRIX_*
_DIRS = {"out": 0, "in": 1}
_I32_MAX = 2 ** 31 - 1


def _dir_code(dir):
    code = _DIRS.get(dir) if isinstance(dir, str) else None
    if code is None:
        raise _arg_error(f"dir must be 'out' or 'in', not {dir!r}")
    return code


class GraphMatrix:
    """A coalesced sparse N x N float32 matrix on the device: `rows`, `cols` (int32) and `values` (float32) of its `nnz` entries, sorted
    by row, then column, each (row, col) at most once; `row_ptr` (int32[N + 1]) delimits the rows."""

    def __init__(self, n, rows, cols, values, row_ptr, num_graphs=1, graph_indicator=None):
        self.shape = (int(n), int(n))
        self.rows, self.cols, self.values, self.row_ptr = rows, cols, values, row_ptr
        self.num_graphs, self.graph_indicator = num_graphs, graph_indicator
        self._graph = None

    @property
    def nnz(self):
        return int(self.rows.numel())

    def __repr__(self):
        return f"GraphMatrix({self.shape[0]} x {self.shape[1]}, {self.nnz} entries)"

    def to_dense(self):
        """the N x N device tensor (for inspection and tests; gradients flow to `values`)"""
        n = self.shape[0]
        at = self.rows.to(torch.int64) * n + self.cols.to(torch.int64)          # distinct positions: a plain indexed write
        dense = torch.zeros(n * n, dtype=torch.float32, device=self.values.device)
        return dense.index_put((at,), self.values).reshape(n, n)

    def as_graph(self):
        """the GNNGraph on the same nodes with one edge j -> i of weight M[i, j] per entry, so that
        propagate(w_mul_xj, M.as_graph(), "+", xj=X) == X @ M.T for X of shape (D x N).  Cached; its device COO lists are in place."""
        if self._graph is None:
            self._graph = _new_graph(self.cols, self.rows, self.shape[0], self.values.device, num_graphs=self.num_graphs,
                                     indicator=self.graph_indicator, ndata=None, edata=None, gdata=None, edge_weight=self.values)
        return self._graph

    def matmul(self, X):
        """M applied to every feature row of X (D x N): X @ M.T = propagate(e_mul_xj, M.as_graph(), "+", xj=X, e=M.values), one fused
        launch with the existing pullback for X and for the values.  propagate(w_mul_xj, M.as_graph(), "+", xj=X) is the same launch
        and gives the same result, but reads the graph's weights as constants (as it does for every graph), so the values would get
        no gradient through it; hence e_mul_xj here."""
        return propagate(e_mul_xj, self.as_graph(), "+", xj=X, e=self.values)

    def diagonal(self):
        """the (N,) float32 diagonal, 0 where the diagonal position is no entry; gradients flow to `values` (distinct positions: a plain
        indexed write)"""
        on = self.rows == self.cols
        out = torch.zeros(self.shape[0], dtype=torch.float32, device=self.values.device)
        return out.index_put((self.rows[on].to(torch.int64),), self.values[on])

    def solve(self, B, **kw):
        """X (D x N) with (shift I + scale M) X[d] = B[d]: linsolve.cg_solve(self, B, **kw), conjugate gradients on the device"""
        from .linsolve import cg_solve
        return cg_solve(self, B, **kw)


class _Assembly:
    """what one ngpde_coo_matrix call wrote: the matrix's structure and what the pullback to the edge weights reads"""

    def __init__(self, g, kind, dir, add_self_loops, w, scale, want_tol):
        dev = _device()
        lib = _lib.load()
        s, t = _coo(g, dev)
        n, e = g.num_nodes, g.num_edges
        m = e + (0 if kind == ADJ else n)
        self.kind, self.n, self.e, self.dev = kind, n, e, dev
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        f32 = lambda k: torch.empty(k, dtype=torch.float32, device=dev)
        rows, cols, vals, self.row_ptr = i32(m), i32(m), f32(m), i32(n + 1)
        group_ptr, member, self.group_of = i32(m + 1), i32(m), i32(m)
        adj, tol = f32(m), (f32(m) if want_tol else None)
        self.deg = None if kind == ADJ else f32(n)
        self.graph_of = None
        if g.num_graphs > 1 and g.graph_indicator is not None:
            self.graph_of = torch.as_tensor(np.ascontiguousarray(g.graph_indicator, dtype=np.int32), device=dev)
        if scale is not None and g.num_graphs > 1 and self.graph_of is None:
            raise _arg_error(f"the graph holds {g.num_graphs} graphs but no graph_indicator: build it with batch(), radius_graph / "
                             "knn_graph(..., graph_indicator=) or GNNGraph(..., graph_indicator=)")
        self.scale = scale
        nnz = C.c_int64(0)
        _lib.check(lib.ngpde_coo_matrix(n, e, _lib.ptr(s), _lib.ptr(t), 0, kind, dir, int(bool(add_self_loops)), _lib.ptr(w), g.num_graphs,
                                        _lib.ptr(self.graph_of), _lib.ptr(scale), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals),
                                        _lib.ptr(self.row_ptr), _lib.ptr(group_ptr), _lib.ptr(member), _lib.ptr(self.group_of), _lib.ptr(adj),
                                        _lib.ptr(self.deg), _lib.ptr(tol), C.byref(nnz), _lib.current_stream()))
        k = self.nnz = int(nnz.value)
        self.rows, self.cols, self.vals, self.adj = rows[:k], cols[:k], vals[:k], adj[:k]
        self.tol = None if tol is None else tol[:k]


class _MatrixFn(torch.autograd.Function):
    """w (E,) -> the values of the assembled matrix.  The pullback is atomic-free and gives the same bits on every run: every step is
    element-wise, an indexed read (group_of: the entry an edge fell into; the entry of a row's diagonal), or the library's ordered
    weighted degree over the matrix's own sorted lists (ngpde_coo_degree: a row's, then a column's entries, front to back)."""

    @staticmethod
    def forward(ctx, w, g, kind, dir, add_self_loops, scale, box):
        a = box[0] = _Assembly(g, kind, dir, add_self_loops, w.detach().contiguous(), scale, False)
        ctx.a = a
        return a.vals

    @staticmethod
    def backward(ctx, dv):
        a = ctx.a
        dv = dv.contiguous()
        rows, cols = a.rows.to(torch.int64), a.cols.to(torch.int64)
        group_of = a.group_of.to(torch.int64)
        if a.kind == ADJ:
            da = dv
        elif a.kind == LAPLACIAN:
            da = dv[group_of[a.e:]][rows] - dv             # d_i feeds the diagonal entry of row i; a feeds its own entry with -1
        else:
            c = 1.0 / torch.sqrt(a.deg)
            q = dv * c[rows] * c[cols]
            if a.scale is not None:
                sc = 2.0 / a.scale
                q = q * (sc[a.graph_of.to(torch.int64)][rows] if a.graph_of is not None else sc[0])
            u = (q * a.adj).contiguous()
            both = torch.empty(a.n, dtype=torch.float32, device=dv.device)     # per node: its row's u, then its column's, in order
            _lib.check(_lib.load().ngpde_coo_degree(a.n, a.nnz, _lib.ptr(a.rows), _lib.ptr(a.cols), 0, 2, _lib.ptr(u), None, _lib.ptr(both),
                                                    _lib.current_stream()))
            da = (0.5 * c * c * both)[rows] - q
        return da[group_of[:a.e]], None, None, None, None, None, None


def _matrix(g, kind, dir, add_self_loops=False, weighted=True, scale=None, want_tol=False, grad=True):
    code = _dir_code(dir)
    w = _edge_weight_of(g) if weighted else None
    if w is not None:
        w = _f32_device(w, _device()).reshape(-1)
    if w is not None and grad and w.requires_grad and torch.is_grad_enabled():
        box = [None]
        vals = _MatrixFn.apply(w, g, kind, code, add_self_loops, scale, box)
        a = box[0]
    else:
        a = _Assembly(g, kind, code, add_self_loops, None if w is None else w.detach().contiguous(), scale, want_tol)
        vals = a.vals
    m = GraphMatrix(g.num_nodes, a.rows, a.cols, vals, a.row_ptr, g.num_graphs, g.graph_indicator)
    return m, a


def adjacency_matrix(g, dir="out", weighted=True):
    """[UPSTREAM GNNGraphs.adjacency_matrix(g; dir, weighted)] A[s, t] = the sum over all edges s -> t of their weight, added in COO order
    (ones with weighted=False or on a graph without `edge_weight`: the multiplicity); dir="in" gives the transpose.  Only existing
    pairs are entries."""
    return _matrix(g, ADJ, dir, weighted=weighted)[0]


def laplacian_matrix(g, dir="out"):
    """[UPSTREAM GNNGraphs.laplacian_matrix(g; dir)] L = D - A with A = adjacency_matrix(g, dir) and D = diag(row sums of A).  Every
    diagonal position is an entry, also where its value is 0 (an isolated node; a node whose only edge is a self loop); existing self
    loops merge into the diagonal, L[i, i] = d_i - a_ii."""
    return _matrix(g, LAPLACIAN, dir)[0]


def normalized_laplacian(g, add_self_loops=False, dir="out"):
    """[UPSTREAM GNNGraphs.normalized_laplacian(g; add_self_loops, dir)] I - D^-1/2 A~ D^-1/2 with A~ = A (+ I) and D = diag(row sums of
    A~); all N diagonal positions are entries.  A row sum that is not positive is an ArgumentError (found on the device by the launch
    that adds the rows; no value is written through it)."""
    return _matrix(g, NORM_LAPLACIAN, dir, add_self_loops=add_self_loops)[0]


def _check_lambda(lambda_max, num_graphs):
    """a user-given lambda_max as a float32 list of num_graphs values, each finite and > 0"""
    if isinstance(lambda_max, torch.Tensor):
        lambda_max = lambda_max.detach().cpu().numpy()
    try:
        lam = np.asarray(lambda_max, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        lam = np.array([np.nan])
    if isinstance(lambda_max, (bool, np.bool_, str, bytes)) or not np.all(np.isfinite(lam)) or not np.all(lam > 0) or lam.size not in (1, num_graphs):
        raise _arg_error(f"lambda_max must be finite and > 0 (one value, or one per graph of the batch), not {lambda_max!r}")
    return np.ascontiguousarray(np.broadcast_to(lam, (num_graphs,)), dtype=np.float32)


def scaled_laplacian(g, dir="out", lambda_max=None):
    """[UPSTREAM GNNGraphs.scaled_laplacian(g; dir)] 2 / lambda_max * Lhat - I with Lhat = normalized_laplacian(g, dir=dir): the spectrum
    moved into [-1, 1], the operator of Chebyshev-polynomial filters.  lambda_max comes from laplacian_lambda_max(g, dir=dir) when not
    given and is a constant for autograd; on a batch every block is scaled by its own graph's value (lambda_max: one value, or one per
    graph)."""
    _dir_code(dir)
    if lambda_max is None:
        lam = laplacian_lambda_max(g, dir=dir)
        lam = lam if isinstance(lam, torch.Tensor) else torch.full((1,), lam, dtype=torch.float32, device=_device())
    else:
        lam = torch.as_tensor(_check_lambda(lambda_max, g.num_graphs), device=_device())
    return _matrix(g, NORM_LAPLACIAN, dir, scale=lam.contiguous())[0]


class LambdaMaxInfo:
    """what laplacian_lambda_max(..., return_info=True) adds: `residual` = |Lhat y - theta y| of the unit Ritz vector y (one more product
    on the device), `iterations` = the Lanczos steps taken -- both per graph (a float / an int for one graph, device tensors for a
    batch) -- and `vector` = y, N floats on the device"""

    def __init__(self, residual, iterations, vector):
        self.residual, self.iterations, self.vector = residual, iterations, vector


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def laplacian_lambda_max(g, add_self_loops=False, dir="out", max_iter=64, tol=1e-5, seed=0, return_info=False):
    """[UPSTREAM GNNGraphs.laplacian_lambda_max(g; add_self_loops, dir)] the largest eigenvalue of normalized_laplacian(g, add_self_loops,
    dir): a Python float for one graph, a float32 device tensor of num_graphs values for a batch (per graph, as upstream returns it).
    A Lanczos iteration with full reorthogonalisation that stays on the device (ngpde_csr_lambda_max), at most max_iter steps per
    graph, stopped when the Ritz value's error bound falls below tol * value; the start vector is a fixed function of `seed`, so the
    result is a pure function of the graph and the arguments.

    The matrix must be symmetric: the coalesced structure equal to its transpose, and a_ij, a_ji equal to within the rounding of their
    two duplicate sums ((m - 1) * 2^-23 * sum |w| each; two single edges must carry the same weight exactly).  Anything else is an
    ArgumentError that names the first offending pair.  On a batch, graph_indicator must be non-decreasing (batch() and radius_graph
    make it so)."""
    code = _dir_code(dir)
    if not _is_int(max_iter) or max_iter < 1:
        raise _arg_error(f"max_iter must be an integer >= 1, not {max_iter!r}")
    if isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (int, float, np.integer, np.floating)) or not math.isfinite(tol) or tol < 0:
        raise _arg_error(f"tol must be a finite number >= 0, not {tol!r}")
    if not _is_int(seed) or not 0 <= seed < 2 ** 64:
        raise _arg_error(f"seed must be an integer in 0 : 2^64 - 1, not {seed!r}")
    gi = g.graph_indicator
    if g.num_graphs > 1 and gi is None:
        raise _arg_error(f"the graph holds {g.num_graphs} graphs but no graph_indicator: build it with batch(), radius_graph / "
                         "knn_graph(..., graph_indicator=) or GNNGraph(..., graph_indicator=)")
    if gi is not None and np.any(np.diff(gi) < 0):
        raise _arg_error("graph_indicator must be non-decreasing (the nodes of a graph contiguous), as batch() and radius_graph make it")
    with torch.no_grad():
        m, a = _matrix(g, NORM_LAPLACIAN, dir, add_self_loops=add_self_loops, want_tol=True, grad=False)
    lib, dev, n, ng = _lib.load(), a.dev, g.num_nodes, g.num_graphs
    _lib.check(lib.ngpde_csr_check_symmetric(n, a.nnz, _lib.ptr(a.row_ptr), _lib.ptr(a.rows), _lib.ptr(a.cols), _lib.ptr(a.adj), _lib.ptr(a.tol),
                                             _lib.current_stream()))
    lam = torch.empty(ng, dtype=torch.float32, device=dev)
    res = torch.empty(ng, dtype=torch.float32, device=dev)
    its = torch.empty(ng, dtype=torch.int32, device=dev)
    vec = torch.empty(n, dtype=torch.float32, device=dev) if return_info else None
    nbytes = int(lib.ngpde_csr_lambda_max_workspace_bytes(n, ng, int(max_iter)))
    if nbytes == 0:
        raise _arg_error(f"max_iter {max_iter} is more than the 4096 steps the iteration supports")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.ngpde_csr_lambda_max(n, a.nnz, _lib.ptr(a.row_ptr), _lib.ptr(a.cols), _lib.ptr(a.vals), ng, _lib.ptr(a.graph_of),
                                        int(max_iter), float(tol), int(seed), _lib.ptr(lam), _lib.ptr(res), _lib.ptr(its), _lib.ptr(vec),
                                        _lib.ptr(ws), nbytes, _lib.current_stream()))
    if ng == 1:
        lam, res, its = float(lam.item()), float(res.item()), int(its.item())
    return (lam, LambdaMaxInfo(res, its, vec)) if return_info else lam


def khop_adj(g, k, dir="out", weighted=True):
    """[UPSTREAM GNNGraphs.khop_adj(g, k; dir, weighted)] A^k as a GraphMatrix: P_1 = A = adjacency_matrix(g, dir, weighted), P_j = P_(j-1) A
    (ngpde_csr_spgemm: expand, sort, combine; an entry's terms are added in ascending middle index, so the result is bitwise
    reproducible).  The structure is that of the boolean product: an entry whose terms cancel to 0.0 stays an entry.  Unlike upstream,
    the values come out with requires_grad = False: no gradient flows through khop_adj."""
    if not _is_int(k) or k < 1:
        raise _arg_error(f"k must be an integer >= 1, not {k!r}")
    _dir_code(dir)
    with torch.no_grad():
        a = _matrix(g, ADJ, dir, weighted=weighted, grad=False)[0]
    a.values = a.values.detach()
    p = a
    lib, n = _lib.load(), g.num_nodes
    for _ in range(int(k) - 1):
        total = C.c_int64(0)
        dev = a.values.device
        off = torch.empty(p.nnz + 1, dtype=torch.int64, device=dev)          # the scanned counts: the product counts nothing again
        _lib.check(lib.ngpde_csr_spgemm_count(n, p.nnz, _lib.ptr(p.cols), a.nnz, _lib.ptr(a.row_ptr), _I32_MAX, _lib.ptr(off), C.byref(total),
                                              _lib.current_stream()))
        m = int(total.value)
        rows = torch.empty(m, dtype=torch.int32, device=dev)
        cols = torch.empty(m, dtype=torch.int32, device=dev)
        vals = torch.empty(m, dtype=torch.float32, device=dev)
        row_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        nnz = C.c_int64(0)
        _lib.check(lib.ngpde_csr_spgemm(n, p.nnz, _lib.ptr(p.rows), _lib.ptr(p.cols), _lib.ptr(p.values), a.nnz, _lib.ptr(a.row_ptr),
                                        _lib.ptr(a.cols), _lib.ptr(a.values), _lib.ptr(off), m, _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals),
                                        _lib.ptr(row_ptr), C.byref(nnz), _lib.current_stream()))
        q = int(nnz.value)
        p = GraphMatrix(n, rows[:q], cols[:q], vals[:q], row_ptr, g.num_graphs, g.graph_indicator)
    return p


def has_isolated_nodes(g, dir="out"):
    """[UPSTREAM GNNGraphs.has_isolated_nodes(g; dir)] true if some node has no edge leaving it (dir="out") or entering it ("in"): one
    read-back over the degree counts"""
    _dir_code(dir)
    return bool((degree(g, dir, edge_weight=False) == 0).any().item())
