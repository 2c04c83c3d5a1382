"""Queries by node and by pair, and the random-walk encoding: the part of GNNGraphs the reference re-exports (src/NeuralGraphPDE.jl:4)
that answers the questions a script asks between `radius_graph`, `sample_neighbors`, `negative_sample` and `updategraph` -- `has_edge`,
`neighbors` / `inneighbors` / `outneighbors`, `adjacency_list`, `intersect` -- and `random_walk_pe`:

    has_edge(g, neg.edge_index()[0], neg.edge_index()[1]).any()        # a negative sample holds no edge of g
    shared = intersect(radius_graph(p, 0.1), radius_graph(p, 0.2))     # the edges two neighbour graphs share
    len(neighbors(g, hub))                                             # a hub's row, before a plan bound is chosen
    pe = random_walk_pe(g, 8)                                          # (8 x N): the return probabilities of walks of 1 .. 8 steps

Node and edge positions are 0-based, as in graphops.py.  Everything runs on the device over the int32 COO lists (include/ngpde.h,
"graph queries by node and by pair"; csrc/graph_query.hip); there is no CPU fallback.  `has_edge` and `intersect` read the graph's
sorted-key plan -- one stable radix sort of the 64-bit keys s * N + t with the COO positions, kept with the structure: a second query
on the same graph sorts nothing.  Every result is bitwise equal from run to run.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .graphops import _arg_error, _coo, _device, _new_graph
from .matrices import GraphMatrix, _dir_code, _is_int, adjacency_matrix

_I64_MAX = 2 ** 63 - 1


class _KeyPlan:
    """what ngpde_coo_sort_keys wrote: the structure's keys s * N + t ascending (their 64 bits in an int64 tensor) and the COO position
    of every sorted key; equal keys ascend by position"""

    def __init__(self, g, dev):
        s, t = _coo(g, dev)
        e = g.num_edges
        self.keys = torch.empty(e, dtype=torch.int64, device=dev)
        self.positions = torch.empty(e, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().ngpde_coo_sort_keys(g.num_nodes, e, _lib.ptr(s), _lib.ptr(t), 0, _lib.ptr(self.keys), _lib.ptr(self.positions),
                                                   _lib.current_stream()))


def _key_plan(g, dev):
    """the structure's plan on `dev`, shared by every copy of the graph (as the readout plan is)"""
    key = ("keyplan", str(dev))
    p = g._shared.get(key)
    if p is None:
        p = g._shared[key] = _KeyPlan(g, dev)
    return p


def _mismatch(msg):
    return _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, "DimensionMismatch: " + msg)


def _ids(v, dev, what):
    """an integer sequence / tensor as an int64 list on the device"""
    if isinstance(v, torch.Tensor):
        if v.dtype in (torch.bool,) or v.is_floating_point() or v.is_complex():
            raise _arg_error(f"{what} must hold integers, not {v.dtype}")
        return v.reshape(-1).to(dev, torch.int64).contiguous()
    a = np.asarray(v)
    if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
        raise _arg_error(f"{what} must hold integers, not {a.dtype}")
    return torch.as_tensor(a.astype(np.int64).reshape(-1), device=dev)


def has_edge(g, s, t, return_eid=False):
    """[UPSTREAM Graphs.has_edge(g, s, t)] is s -> t an edge of g?  Two ints give a Python bool; two integer sequences / tensors of equal
    length give a bool tensor on the device, one element per query.  With return_eid=True the answer is the smallest COO position of
    an edge s -> t, or -1: an int for two ints, else an int32 device tensor.  One lane per query bisects the graph's sorted-key plan.
    A query end outside 0 : N - 1 is a DimensionMismatch that names it (found by the same launch).  The tensor form allocates nothing
    but its outputs and can be captured into a HIP graph once the plan exists; inside a capture nothing is read back, so a bad end
    is not raised there (it answers False / -1)."""
    single = _is_int(s) and _is_int(t)
    if single:
        for v in (s, t):
            if not -_I64_MAX - 1 <= int(v) <= _I64_MAX:
                raise _mismatch(f"has_edge: node {v} lies outside the {g.num_nodes} nodes")
        s, t = [int(s)], [int(t)]
    elif _is_int(s) or _is_int(t):
        raise _arg_error("has_edge: s and t are two ints or two sequences of equal length")
    dev = _device()
    qs, qt = _ids(s, dev, "has_edge: s"), _ids(t, dev, "has_edge: t")
    if qs.numel() != qt.numel():
        raise _arg_error(f"has_edge: s has {qs.numel()} entries and t {qt.numel()}")
    plan = _key_plan(g, dev)
    q = int(qs.numel())
    found = None if return_eid else torch.empty(q, dtype=torch.bool, device=dev)
    eid = torch.empty(q, dtype=torch.int32, device=dev) if return_eid else None
    status = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().ngpde_coo_has_edge(g.num_nodes, g.num_edges, _lib.ptr(plan.keys), _lib.ptr(plan.positions), q, _lib.ptr(qs),
                                              _lib.ptr(qt), 0, _lib.ptr(found), _lib.ptr(eid), _lib.ptr(status), _lib.current_stream()))
    out = eid if return_eid else found
    if single:
        return int(out.item()) if return_eid else bool(out.item())
    return out


class AdjacencyList:
    """[UPSTREAM GNNGraphs.adjacency_list: Vector{Vector{Int}}] a ragged list of rows on the device: row i is
    `neighbors[ptr[i] : ptr[i + 1]]`, the other ends of the edges of the i-th listed node in COO order, and `eid` holds the COO
    positions of those edges (all int32).  `len(al)` is the number of rows, `al[i]` row i as a view of `neighbors`, `al.tolist()`
    the rows as Python lists."""

    def __init__(self, ptr, neighbors, eid):
        self.ptr, self.neighbors, self.eid = ptr, neighbors, eid
        self._host_ptr = None

    def _bounds(self):
        if self._host_ptr is None:
            self._host_ptr = self.ptr.cpu().numpy()
        return self._host_ptr

    def __len__(self):
        return int(self.ptr.numel()) - 1

    def __getitem__(self, i):
        if not _is_int(i):
            raise TypeError(f"row positions are integers, not {type(i).__name__}")
        n = len(self)
        if not -n <= i < n:
            raise IndexError(f"row {i} of an adjacency list of {n} rows")
        p = self._bounds()
        i = int(i) % n
        return self.neighbors[int(p[i]):int(p[i + 1])]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __repr__(self):
        return f"AdjacencyList({len(self)} rows, {int(self.neighbors.numel())} neighbours)"

    def tolist(self):
        p, nb = self._bounds(), self.neighbors.cpu().numpy()
        return [nb[p[i]:p[i + 1]].tolist() for i in range(len(self))]


def adjacency_list(g, nodes=None, dir="out"):
    """[UPSTREAM GNNGraphs.adjacency_list(g, nodes; dir)] for every listed node (0-based; in the order given, a node listed twice gets two
    rows; None: every node) the other ends of its outgoing (dir="out") or incoming ("in") edges, in COO order, parallel edges repeated
    and self loops included: an AdjacencyList on the device.  The by-node rows are those sample_neighbors builds; a count pass sizes
    the result and a second launch fills it with one lane per neighbour, so a hub's row costs no more than its share.  A listed node
    outside 0 : N - 1 is a DimensionMismatch that names it."""
    code = _dir_code(dir)
    dev = _device()
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    listed = None if nodes is None else _ids(nodes, dev, "adjacency_list: nodes")
    if listed is not None and listed.numel() == 0:          # (the C entries read an absent list as every node)
        return AdjacencyList(torch.zeros(1, dtype=torch.int32, device=dev), i32(0), i32(0))
    lib = _lib.load()
    s, t = _coo(g, dev)
    n, e = g.num_nodes, g.num_edges
    n_listed = 0 if listed is None else int(listed.numel())
    row_ptr, row_eid, ptr = i32(n + 1), i32(e), i32((n if listed is None else n_listed) + 1)
    total = C.c_int64(0)
    _lib.check(lib.ngpde_coo_adjacency_count(n, e, _lib.ptr(s), _lib.ptr(t), 0, code, n_listed, _lib.ptr(listed), _lib.ptr(row_ptr),
                                             _lib.ptr(row_eid), _lib.ptr(ptr), C.byref(total), _lib.current_stream()))
    m = int(total.value)
    neighbors, eid = i32(m), i32(m)
    _lib.check(lib.ngpde_coo_adjacency_fill(n, e, _lib.ptr(s), _lib.ptr(t), code, n_listed, _lib.ptr(listed), _lib.ptr(row_ptr), _lib.ptr(row_eid),
                                            _lib.ptr(ptr), m, _lib.ptr(neighbors), _lib.ptr(eid), _lib.current_stream()))
    return AdjacencyList(ptr, neighbors, eid)


def neighbors(g, i, dir="out"):
    """[UPSTREAM Graphs.neighbors(g, i; dir)] the other ends of node i's outgoing (dir="out") or incoming ("in") edges in COO order: an
    int32 device tensor (row 0 of adjacency_list(g, [i], dir))"""
    if not _is_int(i):
        raise _arg_error(f"neighbors: the node is an integer, not {i!r}")
    if not -_I64_MAX - 1 <= int(i) <= _I64_MAX:
        raise _mismatch(f"neighbors: node {i} lies outside the {g.num_nodes} nodes")
    return adjacency_list(g, [int(i)], dir)[0]


def outneighbors(g, i):
    """[UPSTREAM Graphs.outneighbors(g, i)] the targets of node i's outgoing edges, in COO order"""
    return neighbors(g, i, "out")


def inneighbors(g, i):
    """[UPSTREAM Graphs.inneighbors(g, i)] the sources of node i's incoming edges, in COO order"""
    return neighbors(g, i, "in")


def intersect(g1, g2, return_eid=False):
    """[UPSTREAM Base.intersect(g1, g2) on the edge encodings] the graph of the distinct pairs (s, t) that are edges of both graphs, in the
    order of their first appearance in g1's COO list.  Both graphs have the same num_nodes (DimensionMismatch otherwise).  The result
    has g1's num_nodes, num_graphs and graph_indicator, and carries no features and no weights; with return_eid=True
    `edata["EID"]` holds the int64 position in g1 of every kept edge (its first copy), the convention sample_neighbors set."""
    if g1.num_nodes != g2.num_nodes:
        raise _mismatch(f"intersect: the graphs have {g1.num_nodes} and {g2.num_nodes} nodes")
    dev = _device()
    s, t = _coo(g1, dev)
    p1, p2 = _key_plan(g1, dev), _key_plan(g2, dev)
    e = g1.num_edges
    s_out = torch.empty(e, dtype=torch.int32, device=dev)
    t_out = torch.empty(e, dtype=torch.int32, device=dev)
    kept = torch.empty(e, dtype=torch.int64, device=dev)
    n_out = C.c_int64(0)
    _lib.check(_lib.load().ngpde_coo_intersect(g1.num_nodes, e, _lib.ptr(s), _lib.ptr(t), 0, _lib.ptr(p1.keys), _lib.ptr(p1.positions),
                                               g2.num_edges, _lib.ptr(p2.keys), _lib.ptr(s_out), _lib.ptr(t_out), _lib.ptr(kept), C.byref(n_out),
                                               _lib.current_stream()))
    m = int(n_out.value)
    return _new_graph(s_out[:m], t_out[:m], g1.num_nodes, dev, num_graphs=g1.num_graphs, indicator=g1.graph_indicator, ndata=None,
                      edata={"EID": kept[:m]} if return_eid else None, gdata=None, edge_weight=None)


def random_walk_pe(g, walk_length, block=None):
    """[UPSTREAM GNNGraphs.random_walk_pe(g, walk_length)] the random-walk positional encoding: a float32 (walk_length x N) device tensor
    whose row k - 1 holds diag(RW^k), RW = A D^-1 with A = adjacency_matrix(g, dir="out", weighted=True) and D = diag(row sums of A)
    (a node whose row sum is 0 gets 0 everywhere, never inf / nan).  No gradient, as upstream.

    The N seed columns are walked in blocks of `block` consecutive nodes by K sparse products each (ngpde_csr_random_walk_pe: a wave
    per row, its lanes over the block's columns; the step's launch stores the diagonal itself).  On a batch whose graph_indicator
    is non-decreasing a block only touches the rows of the graphs its seeds lie in.  `block` (a multiple of 64; None: the library's
    choice) is for tests and tuning: every sum has a fixed order, so the bits depend neither on it nor on whether a graph is solved
    alone or inside a batch.

    `g` may also be the GraphMatrix adjacency_matrix(g, dir="out") made: nothing is assembled then, the call allocates only through
    torch and can be captured into a HIP graph."""
    if not _is_int(walk_length) or walk_length < 1:
        raise _arg_error(f"walk_length must be an integer >= 1, not {walk_length!r}")
    if block is not None and (not _is_int(block) or block < 64 or block % 64 != 0 or block > 2 ** 30):
        raise _arg_error(f"block must be a multiple of 64 (or None: the library's choice), not {block!r}")
    if isinstance(g, GraphMatrix):
        a = g
    else:
        with torch.no_grad():
            a = adjacency_matrix(g, dir="out", weighted=True)
    lib, n = _lib.load(), a.shape[0]
    dev = a.values.device
    pe = torch.empty((int(walk_length), n), dtype=torch.float32, device=dev)
    if n == 0:
        return pe
    graph_of, n_graphs = None, 1
    if a.num_graphs > 1 and a.graph_indicator is not None and not _lib._capturing():          # (a capture covers all rows: no upload in it)
        graph_of = torch.as_tensor(np.ascontiguousarray(a.graph_indicator, dtype=np.int32), device=dev)
        n_graphs = int(a.num_graphs)
    b = 0 if block is None else int(block)
    nbytes = int(lib.ngpde_csr_random_walk_pe_workspace_bytes(n, b))
    if nbytes == 0:
        raise _arg_error(f"block {block!r}: {n} nodes x block is more state than the walk supports")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.ngpde_csr_random_walk_pe(n, a.nnz, _lib.ptr(a.row_ptr), _lib.ptr(a.cols), _lib.ptr(a.values.detach()), n_graphs,
                                            _lib.ptr(graph_of), int(walk_length), b, _lib.ptr(pe), _lib.ptr(ws), nbytes, _lib.current_stream()))
    return pe
