"""The caller-provided workspaces on the device (csrc/workspace.h: every size query and its entry run ONE layout description).

1. Pinned sizes.  The queries that take a graph handle -- ngpde_gcn_workspace_bytes (forward and pullback),
   ngpde_gcn_backward_ew_workspace_bytes, ngpde_gat_workspace_bytes, ngpde_gat_layer_workspace_bytes,
   ngpde_edge_mlp_backward_workspace_bytes, ngpde_edge_layer_workspace_bytes, ngpde_gno_layer_workspace_bytes -- return what they
   returned before that change on a 70-node graph (two 64-row tiles, three 32-row ones) and on 70 nodes without edges:
   tests/golden/workspace_sizes.json, section "device", recorded on an MI355X from the build before (the persistent grids depend
   on the CU count).
2. Exact fit between guard bands.  Every entry that carves a workspace gets exactly the queried bytes, 4096 bytes into an
   allocation of need + 2 * 4096 sentinel bytes: both bands still hold the sentinel after the call (an overrun is a failed
   assertion here, not a fault), and the outputs are bitwise those of the same call on a workspace twice as large.

The calls go through the package's own functions; a stand-in for the loaded library (Guarded) notes every size query and hands the
entry under test its workspace."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib
from ngpde_amd import functional as F
from ngpde_amd.functional import _int_array, _ptr_array

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAND = 4096
SENTINEL = 0xA5
N = 70
SIZES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")))


class Guarded:
    """The loaded library, except that (a) every *_workspace_bytes call is noted in `queries` as [name, the integer arguments,
    the size] and (b) the entries named in `guard` get a workspace of this object's making in place of the caller's: mode "exact"
    the caller's byte count between two bands of sentinel bytes, checked after the call; mode "double" twice as many bytes."""

    def __init__(self, lib, mode="exact", guard=()):
        self._lib, self._mode, self._guard = lib, mode, set(guard)
        self.queries, self.guarded = [], []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith("_workspace_bytes"):
            types = _lib.SIGNATURES[name][1]

            def query(*args):
                size = int(fn(*args))
                self.queries.append([name, [int(a) for a, ty in zip(args, types) if ty in (C.c_int32, C.c_int64)], size])
                return size
            return query
        if name in self._guard:
            types = _lib.SIGNATURES[name][1]          # (..., workspace, workspace_bytes, stream): the LAST size_t (a seed is one too)
            at = len(types) - 2 - types[::-1].index(C.c_size_t)

            def entry(*args):
                need = int(args[at + 1])
                assert args[at] is not None and need in [q[2] for q in self.queries] + [256], (name, need, self.queries)
                args = list(args)
                if self._mode == "double":
                    buf = torch.full((2 * need,), SENTINEL, dtype=torch.uint8, device=DEV)
                    args[at], args[at + 1] = buf.data_ptr(), 2 * need
                    status = fn(*args)
                else:
                    buf = torch.full((need + 2 * BAND,), SENTINEL, dtype=torch.uint8, device=DEV)
                    args[at] = buf.data_ptr() + BAND
                    status = fn(*args)
                    torch.cuda.synchronize()
                    assert bool((buf[:BAND] == SENTINEL).all()), f"{name}: bytes in front of the workspace were written"
                    assert bool((buf[BAND + need:] == SENTINEL).all()), f"{name}: bytes behind the {need} queried were written"
                self.guarded.append((name, need))
                return status
            return entry
        return fn


def run(monkeypatch, case, mode, guard=()):
    """(outputs, the stand-in) of one case under a stand-in library; the torch draws are those of the test's seed each time"""
    lib = Guarded(_lib.load(), mode, guard)
    with monkeypatch.context() as m:
        m.setattr(_lib, "_lib", lib)
        torch.manual_seed(1234)
        out = case()
        torch.cuda.synchronize()
    return out, lib


def bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


# ---- the graphs -----------------------------------------------------------------------------------------------------------------

def two_rings():
    """70 nodes in two graphs of 35: node j of a graph is joined to j + 1 and j + 5 (mod 35), both ways -- symmetric, in-degree 4"""
    s, t = [], []
    for base in (0, 35):
        for j in range(35):
            for d in (1, 5):
                a, b = base + j, base + (j + d) % 35
                s += [a, b]
                t += [b, a]
    return ng.GNNGraph(s, t, num_nodes=N, index_base=0, graph_indicator=[0] * 35 + [1] * 35, num_graphs=2)


@pytest.fixture(scope="module")
def graphs():
    return {"rings": two_rings(), "edgeless": ng.GNNGraph([], [], num_nodes=N, index_base=0)}


def randn(*shape, grad=True):
    return torch.randn(*shape, device=DEV).requires_grad_(grad)


def grads(y, *leaves):
    y.backward(torch.randn_like(y))
    return [y] + [l.grad for l in leaves]


# ---- the cases: name -> (function of the graph, the entry under guard) ----------------------------------------------------------------

def gcn(din, dout, act="relu"):
    def case(g):
        x, wt, b = randn(N, din), randn(din, dout), randn(dout)
        return grads(F.gcn_conv(x, wt, b, g.handle((True, None, False)), _lib.ACT[act]), x, wt, b)
    return case


def gcn_edge_weight(din, dout):
    def case(g):          # x takes no gradient: the entry gets dx == NULL and keeps the layer's input gradient in its workspace
        x, wt, b = randn(N, din, grad=False), randn(din, dout), randn(dout)
        w = (torch.rand(g.num_edges, device=DEV) + 0.5).requires_grad_(True)
        return grads(F.gcn_conv(x, wt, b, g.handle((True, w.detach(), True)), _lib.ACT["tanh"], w), wt, b, w)
    return case


def dense(n, din, dout, act="tanh"):
    def case(g):
        x, wt, b = randn(n, din), randn(din, dout), randn(dout)
        return grads(F.dense([x], wt, b, _lib.ACT[act]), x, wt, b)
    return case


def gat(heads, c):
    def case(g):
        wx, a = randn(N, heads * c), randn(heads, 2 * c)
        return grads(F.gat_aggregate(wx, a, g.handle((True, None, False)), heads, c, 0.2, g.num_edges), wx, a)
    return case


def gat_layer(heads):
    def case(g):
        c = 64 // heads
        h = g.handle((True, None, False))
        if g.num_edges:
            assert F.gat_layer_supported(h, 64, heads, c)
        else:          # the one-launch layer refuses a graph without edges: only its size query is run there
            _lib.load().ngpde_gat_layer_workspace_bytes(h.ptr, heads, c)
            return []
        x, wt, a, b = randn(N, 64), randn(64, 64), randn(heads, 2 * c), randn(64)
        return grads(F.gat_layer(x, wt, a, b, h, heads, c, 0.2, _lib.ACT["relu"], g.num_edges), x, wt, a, b)
    return case


def edge_mlp(h1, tail):
    """ngpde_edge_mlp_backward through the C ABI (the package reaches it inside ngpde_edge_layer_backward only)"""
    def case(g):
        lib, h = _lib.load(), g.handle()
        douts, acts = _int_array(tail), _int_array([_lib.ACT["tanh"]] * len(tail))
        need = lib.ngpde_edge_mlp_backward_workspace_bytes(h.ptr, h1, len(tail), douts)
        if not g.num_edges:
            return []
        assert lib.ngpde_edge_mlp_backward_supported(h.ptr, h1, len(tail), douts, _lib.AGGR["+"]) == 1
        P, Q, dout = randn(N, h1, grad=False), randn(N, h1, grad=False), randn(N, tail[-1], grad=False)
        W = [randn(a, b, grad=False) for a, b in zip([h1] + tail[:-1], tail)]
        bias = [randn(b, grad=False) for b in tail]
        dP, dQ, dE = torch.empty_like(P), torch.empty_like(Q), torch.empty(g.num_edges, h1, device=DEV)
        dW, db = [torch.empty_like(w) for w in W], [torch.empty_like(b) for b in bias]
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ngpde_edge_mlp_backward(h.ptr, h1, _lib.ACT["tanh"], _lib.ptr(P), _lib.ptr(Q), None, len(tail), douts, acts, _ptr_array(W),
                                               _ptr_array(bias), _lib.AGGR["+"], _lib.ptr(dout), _lib.ptr(dP), _lib.ptr(dQ), _lib.ptr(dE),
                                               _ptr_array(dW), _ptr_array(db), _lib.ptr(ws), need, _lib.current_stream()))
        return [dP, dQ] + dW + db          # (dE: the 64-wide pair sums by source inside its launch and leaves it unwritten)
    return case


def edge_layer(g):
    """VMHConv's shape, forward only, with and without saved activations: the size queries of ngpde_edge_layer_*"""
    x, pos = randn(N, 16), randn(N, 2, grad=False)
    phi = [(randn(34, 64), randn(64), _lib.ACT["tanh"]), (randn(64, 64), randn(64), _lib.ACT["tanh"])]
    upd = [(randn(80, 16), randn(16), _lib.ACT["identity"])]
    y = F.edge_layer(g.handle(), _lib.LAYER_VMH, "+", [x], phi, upd, pos=pos)
    with torch.no_grad():
        F.edge_layer(g.handle(), _lib.LAYER_VMH, "+", [x], phi, upd, pos=pos)
    return [y]


def gno_layer(g):
    h, lwt, lb = randn(N, 16), randn(16, 16), randn(16)
    feat = randn(N, 2, grad=False)
    phi = [(randn(4, 32), randn(32), _lib.ACT["relu"]), (randn(32, 256), randn(256), _lib.ACT["identity"])]
    y = F.gno_layer(g.handle(), 16, 16, _lib.AGGR["mean"], _lib.ACT["relu"], h, lwt, lb, phi, node_feat=feat)
    with torch.no_grad():
        F.gno_layer(g.handle(), 16, 16, _lib.AGGR["mean"], _lib.ACT["relu"], h, lwt, lb, phi, node_feat=feat)
    return [y]


def cg(g):          # two graphs, 65 right-hand sides: one column past a slab of 64
    B = randn(65, N, grad=False)
    X, info = ng.cg_solve(ng.laplacian_matrix(g), B, shift=1.0, return_info=True)
    return [X, info.iterations, info.residual]


def lambda_max(g):
    lam, info = ng.laplacian_lambda_max(g, return_info=True)
    return [lam, info.residual, info.vector]


def random_walk(g):
    return [ng.random_walk_pe(g, 5)]


def hops(g):
    return [ng.hop_distance(g, [0, 40, 7], dir="both", separate=True), ng.hop_distance(g, [3, 69])]


def paths(g):
    w = torch.rand(g.num_edges, device=DEV) + 0.1
    sp = ng.shortest_paths(g, [0, 40, 7], edge_weight=w, dir="both", separate=True, return_parents=True)
    return [sp.dist, sp.parent_eid, sp.parents]


GUARDED = {
    "gcn fused 64 -> 64": (gcn(64, 64), "ngpde_gcn_backward"),
    "gcn any width 12 -> 20": (gcn(12, 20), "ngpde_gcn_backward"),
    "gcn any width 20 -> 12": (gcn(20, 12), "ngpde_gcn_backward"),
    "gcn edge weights, fused, no dx": (gcn_edge_weight(64, 64), "ngpde_gcn_backward_ew"),
    "gcn edge weights 20 -> 12, no dx": (gcn_edge_weight(20, 12), "ngpde_gcn_backward_ew"),
    "dense split-K 64 rows x 512": (dense(64, 48, 512), "ngpde_dense_backward"),
    "dense plain": (dense(N, 48, 40), "ngpde_dense_backward"),
    "gat 2 heads x 12": (gat(2, 12), "ngpde_gat_backward"),
    "gat layer 1 head": (gat_layer(1), "ngpde_gat_layer_backward"),
    "gat layer 4 heads": (gat_layer(4), "ngpde_gat_layer_backward"),
    "edge mlp 64 -> 64": (edge_mlp(64, [64]), "ngpde_edge_mlp_backward"),
    "edge mlp 32 -> 48 -> 24": (edge_mlp(32, [48, 24]), "ngpde_edge_mlp_backward"),
    "cg two graphs, 65 columns": (cg, "ngpde_csr_cg"),
    "lambda max": (lambda_max, "ngpde_csr_lambda_max"),
    "random walk pe": (random_walk, "ngpde_csr_random_walk_pe"),
    "hop distance": (hops, "ngpde_csr_hop_distance"),
    "shortest paths both, separate": (paths, "ngpde_csr_shortest_paths"),
}
# the cases whose size queries take a handle: run on both graphs and compared with the fixture
SIZED = {k: GUARDED[k][0] for k in GUARDED if k.startswith(("gcn", "gat", "edge mlp"))}
SIZED.update({"edge layer": edge_layer, "gno layer": gno_layer})
HANDLE_QUERIES = ("ngpde_gcn_workspace_bytes", "ngpde_gcn_backward_ew_workspace_bytes", "ngpde_gat_workspace_bytes",
                  "ngpde_gat_layer_workspace_bytes", "ngpde_edge_mlp_backward_workspace_bytes", "ngpde_edge_layer_workspace_bytes",
                  "ngpde_gno_layer_workspace_bytes")


def device_sizes(monkeypatch, graphs):
    """{graph: {case: [[query, integer arguments, size], ...]}} of the handle-taking queries, as the library answers now"""
    table = {}
    for gname, g in graphs.items():
        for cname, case in SIZED.items():
            _, lib = run(monkeypatch, lambda: case(g), "exact")
            table.setdefault(gname, {})[cname] = [q for q in lib.queries if q[0] in HANDLE_QUERIES]
    return table


def test_handle_queries_return_the_recorded_sizes(monkeypatch, graphs):
    got = device_sizes(monkeypatch, graphs)
    want = SIZES["device"]
    assert {q[0] for cases in want.values() for qs in cases.values() for q in qs} == set(HANDLE_QUERIES)
    assert got == want, [(g, c, got[g].get(c), want[g][c]) for g in want for c in want[g] if got[g].get(c) != want[g][c]][:4]


@pytest.mark.parametrize("name", list(GUARDED))
def test_exact_fit_between_guard_bands(name, monkeypatch, graphs):
    case, entry = GUARDED[name]
    g = graphs["rings"]
    exact, lib = run(monkeypatch, lambda: case(g), "exact", guard=[entry])
    assert lib.guarded and all(n == entry for n, _ in lib.guarded), lib.guarded          # the entry ran, on the guarded workspace
    double, lib2 = run(monkeypatch, lambda: case(g), "double", guard=[entry])
    assert [n for n, _ in lib2.guarded] == [n for n, _ in lib.guarded]
    assert len(exact) == len(double) > 0
    for k, (a, b) in enumerate(zip(exact, double)):
        if isinstance(a, torch.Tensor):
            assert torch.equal(bits(a), bits(b)), (name, k)
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (name, k)
