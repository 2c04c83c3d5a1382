"""Host-side checks of the queries by node and by pair (queries.py over csrc/graph_query.hip; src/NeuralGraphPDE.jl:4 of the reference
re-exports has_edge, neighbors, adjacency_list, intersect and random_walk_pe with GNNGraphs): the exported names, the argument errors
the package raises before any device call, what the new C entries refuse before they touch the device -- and the numpy restatements
that tests/test_graph_queries_gpu.py compares the device with, pinned here against brute-force Python loops on a 6-node graph.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib

NAMES = ("AdjacencyList", "adjacency_list", "has_edge", "neighbors", "inneighbors", "outneighbors", "intersect", "random_walk_pe")
ENTRIES = ("ngpde_coo_sort_keys", "ngpde_coo_has_edge", "ngpde_coo_adjacency_count", "ngpde_coo_adjacency_fill", "ngpde_coo_intersect",
           "ngpde_csr_random_walk_pe_workspace_bytes", "ngpde_csr_random_walk_pe")
U2 = 2.0 ** -23


# ---- the numpy restatements (the yardstick of the GPU file) -------------------------------------------------------------------

def random_edges(n, e, seed):
    """e random ends with duplicates (the first eighth repeated at the end) and self loops (every seventh edge)"""
    rng = np.random.default_rng(seed)
    s, t = rng.integers(0, n, e), rng.integers(0, n, e)
    k = e // 8
    if k:
        s[-k:], t[-k:] = s[:k], t[:k]
    t[::7] = s[::7]
    return s.astype(np.int64), t.astype(np.int64)


def ref_first_positions(n, s, t):
    """(the distinct keys s * n + t ascending, the smallest COO position of each); int64 holds every key: n < 2^31"""
    return np.unique(np.asarray(s, np.int64) * n + np.asarray(t, np.int64), return_index=True)


def ref_has_edge(n, s, t, qs, qt):
    """(found, eid): eid = the smallest COO position of an edge qs -> qt, or -1"""
    keys, first = ref_first_positions(n, s, t)
    q = np.asarray(qs, np.int64) * n + np.asarray(qt, np.int64)
    at = np.searchsorted(keys, q)
    hit = (at < len(keys)) & (keys[np.minimum(at, max(len(keys) - 1, 0))] == q) if len(keys) else np.zeros(len(q), bool)
    eid = np.where(hit, first[np.minimum(at, max(len(keys) - 1, 0))] if len(keys) else -1, -1)
    return hit, eid.astype(np.int64)


def ref_adjacency(n, s, t, nodes, dir):
    """(ptr, neighbors, eid) of the upstream loop: for every listed node, in the order given, the other ends of its outgoing ("out") or
    incoming ("in") edges in COO order"""
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    own, other = (s, t) if dir == "out" else (t, s)
    order = np.argsort(own, kind="stable")                      # the rows: COO positions grouped by node, COO order inside
    rowptr = np.searchsorted(own[order], np.arange(n + 1))
    nodes = np.arange(n) if nodes is None else np.asarray(nodes, np.int64)
    eid = [order[rowptr[v]:rowptr[v + 1]] for v in nodes]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in eid])]).astype(np.int64)
    eid = np.concatenate(eid).astype(np.int64) if len(eid) else np.zeros(0, np.int64)
    return ptr, other[eid], eid


def ref_intersect(n, s1, t1, s2, t2):
    """(s, t, eid): the distinct pairs of both lists in the order of their first appearance in the first list; eid = that position"""
    k1, first = ref_first_positions(n, s1, t1)
    k2 = np.asarray(s2, np.int64) * n + np.asarray(t2, np.int64)
    both = np.intersect1d(k1, k2)
    eid = np.sort(first[np.searchsorted(k1, both)])
    return np.asarray(s1, np.int64)[eid], np.asarray(t1, np.int64)[eid], eid


def ref_random_walk(n, s, t, w, walk_length):
    """(pe, bound), float64 [walk_length][n], by the dense power: A[s][t] += w, d = the row sums, RW[i][j] = A[i][j] * inv[j] with
    inv[j] = 0 where d[j] == 0; bound[k - 1][i] = k * (m + 3) * 2^-23 * (|RW|^k)[i][i] with |RW| from |A| * |inv| and m the longest row"""
    a = np.zeros((n, n))
    np.add.at(a, (np.asarray(s, np.int64), np.asarray(t, np.int64)), np.ones(len(s)) if w is None else np.asarray(w, np.float64))
    struct = np.zeros((n, n), bool)
    struct[np.asarray(s, np.int64), np.asarray(t, np.int64)] = True
    m = int(struct.sum(1).max()) if len(s) else 0
    d = a.sum(1)
    with np.errstate(divide="ignore"):
        inv = np.where(d == 0, 0.0, 1.0 / np.where(d == 0, 1.0, d))
    rw = a * inv[None, :]
    rw_abs = np.abs(a) * np.abs(inv)[None, :]
    pe, bound = np.zeros((walk_length, n)), np.zeros((walk_length, n))
    p, q = np.eye(n), np.eye(n)
    for k in range(1, walk_length + 1):
        p, q = rw @ p, rw_abs @ q
        pe[k - 1], bound[k - 1] = np.diag(p), k * (m + 3) * U2 * np.diag(q)
    return pe, bound


# ---- the yardstick, pinned by brute force on a 6-node graph ---------------------------------------------------------------------

SIX_S = [0, 1, 1, 2, 0, 1, 4, 4, 2, 1]          # a duplicate (1 -> 2 three times, 0 -> 1 twice), a self loop (4 -> 4), node 5 isolated,
SIX_T = [1, 2, 2, 0, 1, 2, 4, 3, 3, 0]          # node 3 a sink
SIX_W = [1.0, 0.5, 2.0, 1.5, 0.25, 1.0, 3.0, 1.0, 0.75, 2.0]


def test_restated_has_edge_and_intersect_agree_with_brute_force():
    n, s, t = 6, SIX_S, SIX_T
    qs, qt = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    found, eid = ref_has_edge(n, s, t, qs, qt)
    for a, b, f, e in zip(qs, qt, found, eid):
        where = [i for i in range(len(s)) if s[i] == a and t[i] == b]
        assert bool(f) == bool(where) and e == (where[0] if where else -1)
    s2, t2 = [2, 1, 4, 5, 1, 0], [3, 2, 4, 5, 2, 2]
    want = []
    for i in range(len(s)):
        pair = (s[i], t[i])
        if pair in zip(s2, t2) and pair not in [(s[j], t[j]) for j in range(i)]:
            want.append((s[i], t[i], i))
    got = ref_intersect(n, s, t, s2, t2)
    assert [tuple(int(v) for v in r) for r in zip(*got)] == want == [(1, 2, 1), (4, 4, 6), (2, 3, 8)]
    assert len(ref_intersect(n, s, t, [], [])[2]) == 0


def test_restated_adjacency_agrees_with_brute_force():
    n, s, t = 6, SIX_S, SIX_T
    for dir in ("out", "in"):
        for nodes in (None, [4, 1, 5, 1], []):
            ptr, nb, eid = ref_adjacency(n, s, t, nodes, dir)
            listed = range(n) if nodes is None else nodes
            rows = [[(t[i] if dir == "out" else s[i], i) for i in range(len(s)) if (s[i] if dir == "out" else t[i]) == v] for v in listed]
            assert ptr.tolist() == [0] + list(np.cumsum([len(r) for r in rows]))
            assert nb.tolist() == [x for r in rows for x, _ in r] and eid.tolist() == [i for r in rows for _, i in r]
    assert ref_adjacency(n, s, t, [1], "out")[1].tolist() == [2, 2, 2, 0]


def test_restated_random_walk_agrees_with_brute_force():
    n, s, t, w, K = 6, SIX_S, SIX_T, SIX_W, 4
    a = [[0.0] * n for _ in range(n)]
    for i in range(len(s)):
        a[s[i]][t[i]] += w[i]
    d = [sum(row) for row in a]
    rw = [[a[i][j] * (0.0 if d[j] == 0 else 1.0 / d[j]) for j in range(n)] for i in range(n)]
    p = [[float(i == j) for j in range(n)] for i in range(n)]
    pe, bound = ref_random_walk(n, s, t, np.float32(w), K)
    for k in range(K):
        p = [[sum(rw[i][l] * p[l][j] for l in range(n)) for j in range(n)] for i in range(n)]
        assert np.allclose(pe[k], [p[i][i] for i in range(n)], rtol=1e-14, atol=0)
    assert np.all(pe[:, 5] == 0) and np.all(pe[:, 3] == 0) and np.all(np.isfinite(pe))          # the isolated node and the sink
    # m is the longest row of the COALESCED matrix (0 -> {1}, 1 -> {0, 2}, 2 -> {0, 3}, 4 -> {3, 4}): 2; RW[4][4] = 3 / 4
    assert pe[0, 4] == 0.75 and bound[0, 4] == 1 * (2 + 3) * U2 * 0.75 and np.all(bound >= 0)


# ---- names and argument errors ----------------------------------------------------------------------------------------------------

def graph(**kw):
    return ng.GNNGraph([0, 0, 1, 2], [1, 2, 0, 0], num_nodes=3, index_base=0, **kw)


def test_names_are_exported():
    for name in NAMES:
        assert name in ng.__all__, name
        assert callable(getattr(ng, name)), name


def test_entries_are_declared_bound_and_cited():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ngpde.h")).read()
    block = header[header.index("graph queries by node and by pair on a device COO list"):header.index("GNOConv message (src/layers.jl:527-530)")]
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name + "(" in block, name
    assert block.count("src/NeuralGraphPDE.jl:4") >= 6          # the block and each entry's comment cite the re-export
    assert "ASCENDING COLUMN ORDER" in block and "-ffp-contract=off" in block          # the summation order is part of the definition


def test_argument_errors_come_before_any_device_call():
    g = graph()
    for k in (0, -1, 1.5, "2", None, True):
        with pytest.raises(ng.ArgumentError, match="walk_length"):
            ng.random_walk_pe(g, k)
    for block in (0, 1, 63, 65, 100, -64, 64.0, "64", True):
        with pytest.raises(ng.ArgumentError, match="multiple of 64"):
            ng.random_walk_pe(g, 2, block=block)
    for bad in ("both", "IN", 0, None, True):
        with pytest.raises(ng.ArgumentError, match="dir must be"):
            ng.adjacency_list(g, dir=bad)
        with pytest.raises(ng.ArgumentError, match="dir must be"):
            ng.neighbors(g, 0, dir=bad)
    for i in (1.0, "1", None, [1], True):
        with pytest.raises(ng.ArgumentError, match="integer"):
            ng.neighbors(g, i)
    with pytest.raises(ng.ArgumentError, match="two ints or two sequences"):
        ng.has_edge(g, 0, [1])
    with pytest.raises(ng.DimensionMismatch, match="3 and 4 nodes"):
        ng.intersect(g, ng.GNNGraph([0], [1], num_nodes=4, index_base=0))


# ---- the C entries --------------------------------------------------------------------------------------------------------------

ONE = C.c_void_p(16)     # (never dereferenced: the checks come before any device call)


def test_key_plan_and_has_edge_refuse_null_and_negative_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT

    def sort(n=3, e=4, s=ONE, t=ONE, keys=ONE, pos=ONE):
        return lib.ngpde_coo_sort_keys(n, e, s, t, 0, keys, pos, None)

    def has(n=3, e=4, keys=ONE, pos=ONE, q=2, qs=ONE, qt=ONE, found=ONE, eid=ONE, status=ONE):
        return lib.ngpde_coo_has_edge(n, e, keys, pos, q, qs, qt, 0, found, eid, status, None)

    for call in (sort, has):
        for n, e in ((-1, 0), (3, -1)):
            assert call(n=n, e=e) == bad and b"negative" in lib.ngpde_last_error()
        for n, e in ((2 ** 31, 1), (3, 2 ** 31)):
            assert call(n=n, e=e) == bad and b"2^31" in lib.ngpde_last_error()
    for kw in (dict(s=None), dict(t=None), dict(keys=None), dict(pos=None)):
        assert sort(**kw) == bad and b"NULL" in lib.ngpde_last_error()
    assert sort(n=0) == _lib.ERR_DIMENSION_MISMATCH
    assert sort(e=0, s=None, t=None, keys=None, pos=None) == 0          # nothing to sort is not an error
    for q in (-1, 2 ** 31):
        assert has(q=q) == bad and b"n_queries" in lib.ngpde_last_error()
    for kw in (dict(keys=None), dict(pos=None), dict(qs=None), dict(qt=None), dict(found=None, eid=None), dict(status=None)):
        assert has(**kw) == bad and b"NULL" in lib.ngpde_last_error(), kw
    assert has(q=0, qs=None, qt=None, found=None, eid=None, status=None) == 0          # zero queries are valid


def test_adjacency_entries_refuse_null_and_negative_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT

    def count(n=3, e=4, s=ONE, t=ONE, dir=0, n_listed=2, nodes=ONE, outs=(ONE, ONE, ONE), total=True):
        n64 = C.c_int64(7)
        return lib.ngpde_coo_adjacency_count(n, e, s, t, 0, dir, n_listed, nodes, *outs, C.byref(n64) if total else None, None), n64.value

    def fill(n=3, e=4, s=ONE, t=ONE, dir=0, n_listed=2, nodes=ONE, lists=(ONE, ONE, ONE), total=5, outs=(ONE, ONE)):
        return lib.ngpde_coo_adjacency_fill(n, e, s, t, dir, n_listed, nodes, *lists, total, *outs, None), 0

    for call in (count, fill):
        for n, e in ((-1, 0), (3, -1)):
            assert call(n=n, e=e)[0] == bad and b"negative" in lib.ngpde_last_error()
        for n, e in ((2 ** 31, 1), (3, 2 ** 31)):
            assert call(n=n, e=e)[0] == bad and b"2^31" in lib.ngpde_last_error()
        for dir in (-1, 2):
            assert call(dir=dir)[0] == bad and b"dir" in lib.ngpde_last_error()
        for n_listed in (-1, 2 ** 31):
            assert call(n_listed=n_listed)[0] == bad and b"n_listed" in lib.ngpde_last_error()
        assert call(nodes=None)[0] == bad and b"nodes is NULL" in lib.ngpde_last_error()
        assert call(s=None)[0] == bad and b"s / t is NULL" in lib.ngpde_last_error()
    assert count(total=False)[0] == bad and b"total_out is NULL" in lib.ngpde_last_error()
    assert count(n=0) == (_lib.ERR_DIMENSION_MISMATCH, 0)
    for k in range(3):
        outs = [ONE] * 3
        outs[k] = None
        assert count(outs=tuple(outs)) == (bad, 0) and b"NULL" in lib.ngpde_last_error(), k
    for total in (-1, 2 ** 31):
        assert fill(total=total)[0] == bad and b"total" in lib.ngpde_last_error()
    assert fill(total=0, s=None, t=None, lists=(None,) * 3, outs=(None, None))[0] == 0          # nothing to fill is not an error
    assert fill(e=0)[0] == bad and b"without rows or edges" in lib.ngpde_last_error()
    for k in range(3):
        lists = [ONE] * 3
        lists[k] = None
        assert fill(lists=tuple(lists))[0] == bad and b"NULL" in lib.ngpde_last_error(), k
    for outs in ((None, ONE), (ONE, None)):
        assert fill(outs=outs)[0] == bad and b"NULL" in lib.ngpde_last_error()


def test_intersect_refuses_null_and_negative_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT

    def call(n=3, e=4, s=ONE, t=ONE, keys=ONE, pos=ONE, e2=4, keys2=ONE, outs=(ONE, ONE, ONE), out=True):
        n64 = C.c_int64(7)
        return lib.ngpde_coo_intersect(n, e, s, t, 0, keys, pos, e2, keys2, *outs, C.byref(n64) if out else None, None), n64.value

    for kw in (dict(n=-1), dict(e=-1)):
        assert call(**kw)[0] == bad and b"negative" in lib.ngpde_last_error()
    for kw in (dict(n=2 ** 31), dict(e=2 ** 31)):
        assert call(**kw)[0] == bad and b"2^31" in lib.ngpde_last_error()
    for e2 in (-1, 2 ** 31):
        assert call(e2=e2)[0] == bad and b"n_edges2" in lib.ngpde_last_error()
    assert call(out=False)[0] == bad and b"n_out is NULL" in lib.ngpde_last_error()
    for kw in (dict(s=None), dict(t=None), dict(keys=None), dict(pos=None), dict(keys2=None)):
        assert call(**kw) == (bad, 0) and b"NULL" in lib.ngpde_last_error(), kw
    for k in range(3):
        outs = [ONE] * 3
        outs[k] = None
        assert call(outs=tuple(outs)) == (bad, 0) and b"NULL" in lib.ngpde_last_error(), k
    assert call(n=0) == (_lib.ERR_DIMENSION_MISMATCH, 0)
    assert call(e=0, s=None, t=None, keys=None, pos=None, outs=(None,) * 3) == (0, 0)          # an empty first list shares nothing


def test_random_walk_refuses_bad_arguments_and_sizes_its_workspace():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    size = lib.ngpde_csr_random_walk_pe_workspace_bytes

    def walk(n=3, nnz=4, lists=(ONE, ONE, ONE), n_graphs=1, graph_of=None, k=2, block=64, pe=ONE, ws=ONE, ws_bytes=1 << 30):
        return lib.ngpde_csr_random_walk_pe(n, nnz, *lists, n_graphs, graph_of, k, block, pe, ws, ws_bytes, None)

    for n, nnz in ((-1, 0), (3, -1)):
        assert walk(n, nnz) == bad and b"negative" in lib.ngpde_last_error()
    for n, nnz in ((2 ** 31, 1), (3, 2 ** 31)):
        assert walk(n, nnz) == bad and b"2^31" in lib.ngpde_last_error()
    for k in (0, -1):
        assert walk(k=k) == bad and b"walk_length" in lib.ngpde_last_error()
    for block in (-64, 1, 63, 65, 100):
        assert walk(block=block) == bad and b"multiple of 64" in lib.ngpde_last_error()
    assert walk(n_graphs=0) == bad and b"n_graphs" in lib.ngpde_last_error()
    for k in range(3):
        lists = [ONE] * 3
        lists[k] = None
        assert walk(lists=tuple(lists)) == bad and b"NULL" in lib.ngpde_last_error()
    assert walk(pe=None) == bad and b"pe is NULL" in lib.ngpde_last_error()
    assert walk(ws=None) == _lib.ERR_WORKSPACE
    assert walk(ws_bytes=size(3, 64) - 1) == _lib.ERR_WORKSPACE and b"needed" in lib.ngpde_last_error()
    # the header's formula: the two states, then n * 4 rounded up to 256 bytes (the reciprocal row sums) and 256 bytes of flag words
    for n in (0, 1, 63, 64, 65, 300, 16384, 100003):
        for block in (64, 128, 256, 1024):
            assert size(n, block) == 2 * n * block * 4 + (n * 4 + 255) // 256 * 256 + 256, (n, block)
    for n, chosen in ((1, 64), (64, 64), (65, 128), (200, 256), (16384, 256), (72000, 256), (200000, 128)):
        assert size(n, 0) == size(n, chosen), n          # block 0: 256, fewer for fewer nodes or where the states would pass 256 MiB
    for n, block in ((-1, 64), (2 ** 31, 64), (10, -64), (10, 1), (10, 100)):
        assert size(n, block) == 0
