"""The inverse side of a graph matrix: what upstream writes as `A \\ b` or `IterativeSolvers.cg(A, b)` on the SparseMatrixCSC that
`laplacian_matrix` returns there --

    L = laplacian_matrix(g)
    u1 = cg_solve(L, u0, shift=1.0, scale=dt)            # one implicit Euler step of u' = -L u: (I + dt L) u1 = u0, any dt
    u1 = L.solve(u0, shift=1.0, scale=dt)                # the same call as a method
    X, info = cg_solve(L, B, shift=k2, return_info=True) # a screened Poisson solve; info.status / iterations / residual per (graph, column)

`cg_solve` solves (shift I + scale M) x_d = b_d for every feature row d of B (D x N, the layout `matmul` takes) by a conjugate-gradient
iteration that lives on the device (include/ngpde.h, "graph solves"; csrc/graph_solve.hip): three launches per step, every (graph,
column) pair with its own scalars, stop and iteration count, no float atomics, the same bits on every run and whatever else is in the
batch.  There is no CPU fallback and no dense matrix.  Gradients flow to B and to `M.values` (and so, through `laplacian_matrix`'s
pullback, to a float32 `edge_weight`); `shift`, `scale` and `x0` are constants for autograd.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .graphops import _arg_error, _device
from .matrices import GraphMatrix, _is_int
from .msgpass import apply_edges, xi_dot_xj

_PRECONDITION = {None: 0, "jacobi": 1}          # NGPDE_CG_*


class CGInfo:
    """what cg_solve(..., return_info=True) adds, all (num_graphs x D) device tensors: `status` (int32: 0 converged, 1 max_iter reached, 2
    breakdown), `iterations` (int32) and `residual` (float32, the recurrence residual's 2-norm at the stop)"""

    def __init__(self, status, iterations, residual):
        self.status, self.iterations, self.residual = status, iterations, residual

    def __repr__(self):
        return f"CGInfo({tuple(self.status.shape)[0]} graphs x {tuple(self.status.shape)[1]} columns)"


def _number(name, v, lo=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or (lo is not None and v < lo):
        raise _arg_error(f"{name} must be a finite number" + (f" >= {lo}" if lo is not None else "") + f", not {v!r}")
    return float(v)


def _rhs(name, t, n, d=None):
    if not isinstance(t, torch.Tensor):
        raise _arg_error(f"{name} must be a torch tensor, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise _arg_error(f"{name} must hold float32 values, not {t.dtype}")
    if t.dim() != 2 or t.shape[1] != n or t.shape[0] < 1 or (d is not None and t.shape[0] != d):
        want = f"({d if d is not None else 'D'} x {n})"
        raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, f"DimensionMismatch: {name} has shape {tuple(t.shape)}, the matrix takes {want}")
    return t


class _Settings:
    """one call's checked arguments: what the pullback solves with again"""

    def __init__(self, M, shift, scale, rtol, atol, max_iter, precondition, check_every):
        if not isinstance(M, GraphMatrix):
            raise _arg_error(f"cg_solve takes a GraphMatrix, not {type(M).__name__}")
        self.M, self.n = M, M.shape[0]
        self.shift, self.scale = _number("shift", shift), _number("scale", scale)
        self.rtol, self.atol = _number("rtol", rtol, 0), _number("atol", atol, 0)
        if precondition not in _PRECONDITION or isinstance(precondition, (bool, np.bool_)):
            raise _arg_error(f"precondition must be 'jacobi' or None, not {precondition!r}")
        self.precondition = _PRECONDITION[precondition]
        if not _is_int(check_every) or check_every < 0:
            raise _arg_error(f"check_every must be an integer >= 0, not {check_every!r}")
        self.check_every = int(check_every)
        gi = M.graph_indicator
        if M.num_graphs > 1 and gi is None:
            raise _arg_error(f"the matrix holds {M.num_graphs} graphs but no graph_indicator: build its graph with batch(), radius_graph / "
                             "knn_graph(..., graph_indicator=) or GNNGraph(..., graph_indicator=)")
        if gi is not None and np.any(np.diff(np.asarray(gi)) < 0):
            raise _arg_error("graph_indicator must be non-decreasing (the nodes of a graph contiguous), as batch() and radius_graph make it")
        self.gi = None if gi is None or M.num_graphs == 1 else np.ascontiguousarray(gi, dtype=np.int32)
        if max_iter is None:
            largest = self.n if self.gi is None else int(np.bincount(self.gi, minlength=1).max(initial=0))
            max_iter = min(largest, 1000)
        if not _is_int(max_iter) or max_iter < 0:
            raise _arg_error(f"max_iter must be an integer >= 0, not {max_iter!r}")
        self.max_iter = int(max_iter)
        self._graph_of = None

    def graph_of(self, dev):
        if self.gi is not None and self._graph_of is None:
            self._graph_of = torch.as_tensor(self.gi, device=dev)
        return self._graph_of


def _run(s, values, B, x0):
    """the C entry on detached tensors: X and the three info arrays"""
    M, n, d, ng = s.M, s.n, int(B.shape[0]), s.M.num_graphs
    dev = B.device
    lib = _lib.load()
    B = B.contiguous()
    x0 = None if x0 is None else x0.contiguous()
    X = torch.empty_like(B)
    status = torch.empty((ng, d), dtype=torch.int32, device=dev)
    its = torch.empty((ng, d), dtype=torch.int32, device=dev)
    res = torch.empty((ng, d), dtype=torch.float32, device=dev)
    nbytes = int(lib.ngpde_csr_cg_workspace_bytes(n, ng, d))
    if nbytes == 0:
        raise _arg_error(f"{ng} graphs x {d} columns over {n} nodes are more than the iteration holds")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(max_iter, check_every, X, status, its, res):
        return lib.ngpde_csr_cg(n, M.nnz, _lib.ptr(M.row_ptr), _lib.ptr(M.cols), _lib.ptr(values), ng, _lib.ptr(s.graph_of(dev)), s.shift, s.scale,
                                d, _lib.ptr(B), _lib.ptr(x0), _lib.ptr(X), s.precondition, s.rtol, s.atol, max_iter, check_every,
                                _lib.ptr(status), _lib.ptr(its), _lib.ptr(res), _lib.ptr(ws), nbytes, _lib.current_stream())

    _lib.check(call(s.max_iter, s.check_every, X, status, its, res))
    if torch.cuda.is_current_stream_capturing():          # (check_every = 0 inside a capture: the statuses are the caller's to read)
        return X, status, its, res
    broke = (status == 2).nonzero()
    if broke.numel():
        if s.check_every == 0:          # input the device refused leaves every status 2: the checked form of the call names it
            _lib.check(call(0, 1, torch.empty_like(X), torch.empty_like(status), torch.empty_like(its), torch.empty_like(res)))
        g, c = (int(v) for v in broke[0])
        raise _arg_error(f"cg_solve: {s.shift!r} * I + {s.scale!r} * M is not positive definite: graph {g}, column {c} broke down after "
                         f"{int(its[g, c])} iterations (p . Ap <= 0 or a non-finite value)")
    return X, status, its, res


class _SolveFn(torch.autograd.Function):
    """(B, values, x0) -> X.  dB = the same solve of dX (the operator is symmetric); dvalues[(i, j)] = -scale * sum_d dB[d, i] X[d, j], the
    library's one-launch xi_dot_xj over the matrix's graph: no atomics, the same bits on every run; x0 gets no gradient."""

    @staticmethod
    def forward(ctx, B, values, x0, s, box):
        X, *info = _run(s, values.detach(), B.detach(), None if x0 is None else x0.detach())
        box[0] = info
        ctx.s, ctx.values = s, values.detach()
        ctx.save_for_backward(X)
        return X

    @staticmethod
    def backward(ctx, dX):
        (X,), s = ctx.saved_tensors, ctx.s
        dB = _run(s, ctx.values, dX, None)[0]
        dvalues = None
        if ctx.needs_input_grad[1]:
            dvalues = -s.scale * apply_edges(xi_dot_xj, s.M.as_graph(), xi=dB, xj=X).reshape(-1)
        return (dB if ctx.needs_input_grad[0] else None), dvalues, None, None, None


def cg_solve(M, B, *, shift=0.0, scale=1.0, x0=None, rtol=1e-5, atol=0.0, max_iter=None, precondition="jacobi", check_every=16,
             return_info=False, check_symmetric=True):
    """[UPSTREAM `A \\ b` / IterativeSolvers.cg on the SparseMatrixCSC of GNNGraphs.laplacian_matrix] X (D x N) with (shift I + scale M) X[d] =
    B[d] for every feature row d of B (D x N float32 on the device), by conjugate gradients.

    shift I + scale M must be symmetric positive definite.  Symmetry is checked (ngpde_csr_check_symmetric, exact; check_symmetric=False
    skips it).  Definiteness is found out by the iteration: a step with p . Ap <= 0 or a non-finite value stops that column with status
    2, and the call raises ArgumentError ("not positive definite") naming the first such graph and column.  precondition "jacobi"
    divides by the diagonal shift + scale * M[i, i] (a value that is not > 0 is an ArgumentError naming the smallest such node); None
    runs plain CG.  x0 (D x N) is a warm start.  max_iter defaults to min(nodes of the largest graph, 1000); reaching it does not raise
    (status 1).

    On a batch (graph_indicator non-decreasing) every (graph, column) pair is its own CG and stops by itself when |r|_2 <= max(rtol *
    |b|_2, atol), r the recurrence residual; a stopped pair is frozen.  check_every = k > 0: the host reads one word every k steps and
    ends the loop when every pair has stopped; 0: exactly max_iter steps are enqueued without a read-back.  The result does not depend
    on check_every, on D, on the column's place in B, or on the other graphs of the batch -- bitwise.

    return_info=True returns (X, CGInfo)."""
    s = _Settings(M, shift, scale, rtol, atol, max_iter, precondition, check_every)
    B = _rhs("B", B, s.n)
    if x0 is not None:
        x0 = _rhs("x0", x0, s.n, int(B.shape[0]))
    dev = _device()
    if B.device != dev or (x0 is not None and x0.device != dev) or M.values.device != dev:
        raise _arg_error(f"B, x0 and the matrix must live on {dev} (B is on {B.device}): the solve runs on the GPU, there is no CPU fallback")
    if s.n == 0:
        raise _arg_error("cg_solve: the matrix has no rows")
    if check_symmetric:
        with torch.no_grad():
            _lib.check(_lib.load().ngpde_csr_check_symmetric(s.n, M.nnz, _lib.ptr(M.row_ptr), _lib.ptr(M.rows), _lib.ptr(M.cols),
                                                             _lib.ptr(M.values.detach()), None, _lib.current_stream()))
    box = [None]
    if torch.is_grad_enabled() and (B.requires_grad or M.values.requires_grad):
        X = _SolveFn.apply(B, M.values, x0, s, box)
        info = box[0]
    else:
        X, *info = _run(s, M.values.detach(), B.detach(), None if x0 is None else x0.detach())
    return (X, CGInfo(*info)) if return_info else X
