"""Host-side checks of the graph traversal (traversal.py over csrc/graph_traverse.hip; the reference's GNNGraph is a Graphs.AbstractGraph,
src/NeuralGraphPDE.jl:4 / :16, so connected_components, is_connected, gdistances and neighborhood work on it): the exported names, the
argument errors the package raises before any device call, what the new C entries refuse before they touch the device -- and the numpy
restatements that tests/test_traversal_gpu.py compares the device with, pinned here against a brute-force union-find and a deque BFS on
a hand-written 8-node graph (and against scipy.sparse.csgraph where scipy imports).  No GPU."""
import ctypes as C
import os
from collections import deque

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib

NAMES = ("Components", "connected_components", "is_connected", "split_components", "hop_distance", "neighborhood")
ENTRIES = ("ngpde_coo_components_workspace_bytes", "ngpde_coo_components", "ngpde_components_rank", "ngpde_coo_rows",
           "ngpde_csr_hop_distance_workspace_bytes", "ngpde_csr_hop_distance", "ngpde_hop_reached_nodes")


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


def path_edges(numbering):
    """the path whose k-th node carries the id numbering[k]"""
    numbering = np.asarray(numbering, np.int64)
    return numbering[:-1].copy(), numbering[1:].copy()


def ref_components(n, s, t):
    """(labels, rounds): synchronous min-hooking with full compression.  labels[i] = the smallest member of i's component.  A round:
    every edge reads the roots of its ends as they were when the round began and, where they differ, lowers parent[larger root] to
    the smaller (the minimum over all such edges); then every node is brought to its root.  A round counts even when it hooks nothing:
    the final, confirming round is included."""
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    parent = np.arange(n, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        ra, rb = parent[s], parent[t]
        differ = ra != rb
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        if not differ.any():
            return parent, rounds


def ref_rank(labels):
    """(rank, count, sizes, ptr, order) of the components ranked by their smallest member; order groups the nodes by component,
    ascending inside it"""
    labels = np.asarray(labels, np.int64)
    roots = np.flatnonzero(labels == np.arange(len(labels)))
    rank = np.searchsorted(roots, labels)
    order = np.argsort(rank, kind="stable")
    sizes = np.bincount(rank, minlength=len(roots))
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    return rank, len(roots), sizes, ptr, order


def ref_hop_distance(n, s, t, sources, dir="out", max_hops=None, separate=False):
    """the level loop: dist[v] = the edges on a shortest path from the nearest source, -1 where there is none within max_hops; with
    separate one row per listed source"""
    sources = np.asarray(sources, np.int64).reshape(-1)
    if separate:
        rows = [ref_hop_distance(n, s, t, [v], dir, max_hops) for v in sources]
        return np.stack(rows) if rows else np.zeros((0, n), np.int64)
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    if dir == "in":
        s, t = t, s
    elif dir == "both":
        s, t = np.concatenate([s, t]), np.concatenate([t, s])
    dist = np.full(n, -1, np.int64)
    dist[sources] = 0
    frontier = dist == 0
    level = 0
    while frontier.any() and (max_hops is None or level < max_hops):
        level += 1
        reach = np.zeros(n, bool)
        reach[t[frontier[s]]] = True
        frontier = reach & (dist < 0)
        dist[frontier] = level
    return dist


def ref_split(n, s, t):
    """(s', t', nid, indicator, count): the nodes regrouped by component -- node k of the result is node nid[k] -- the edges in COO order"""
    labels, _ = ref_components(n, s, t)
    rank, count, _, _, order = ref_rank(labels)
    new_id = np.empty(n, np.int64)
    new_id[order] = np.arange(n)
    return new_id[np.asarray(s, np.int64)], new_id[np.asarray(t, np.int64)], order, rank[order], count


# ---- the yardstick, pinned by brute force on an 8-node graph --------------------------------------------------------------------

# two components with edges -- {0, 3, 5, 6} and {1, 2, 7} --, a self loop (5 -> 5), a parallel edge (3 -> 0 twice), node 4 isolated
EIGHT_S = [3, 6, 3, 5, 7, 2, 5, 1]
EIGHT_T = [0, 3, 0, 5, 2, 1, 6, 7]


def brute_components(n, s, t):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in zip(s, t):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return [find(x) for x in range(n)]


def brute_bfs(n, s, t, sources, dir, max_hops):
    nbrs = [[] for _ in range(n)]
    for a, b in zip(s, t):
        if dir in ("out", "both"):
            nbrs[a].append(b)
        if dir in ("in", "both"):
            nbrs[b].append(a)
    dist = [-1] * n
    queue = deque()
    for v in sources:
        if dist[v] < 0:
            dist[v] = 0
            queue.append(v)
    while queue:
        v = queue.popleft()
        if max_hops is not None and dist[v] >= max_hops:
            continue
        for u in nbrs[v]:
            if dist[u] < 0:
                dist[u] = dist[v] + 1
                queue.append(u)
    return dist


def test_restated_components_agree_with_union_find():
    n, s, t = 8, EIGHT_S, EIGHT_T
    labels, rounds = ref_components(n, s, t)
    assert labels.tolist() == brute_components(n, s, t) == [0, 1, 1, 0, 4, 0, 0, 1]
    assert rounds >= 2                                                    # at least one hooking round and the confirming one
    rank, count, sizes, ptr, order = ref_rank(labels)
    assert count == 3 and rank.tolist() == [0, 1, 1, 0, 2, 0, 0, 1]
    assert sizes.tolist() == [4, 3, 1] and ptr.tolist() == [0, 4, 7, 8] and order.tolist() == [0, 3, 5, 6, 1, 2, 7, 4]
    assert ref_components(3, [], [])[0].tolist() == [0, 1, 2] and ref_components(3, [], [])[1] == 1      # no edges: the confirming round alone
    s2, t2, nid, indicator, k = ref_split(n, s, t)
    assert k == 3 and nid.tolist() == order.tolist() and indicator.tolist() == [0, 0, 0, 0, 1, 1, 1, 2]
    assert np.array_equal(nid[s2], s) and np.array_equal(nid[t2], t)          # the edges are those of g, in COO order


def test_restated_hop_distance_agrees_with_deque_bfs():
    n, s, t = 8, EIGHT_S, EIGHT_T
    for dir in ("out", "in", "both"):
        for sources in ([6], [7, 6, 7], list(range(n)), [], [4]):
            for max_hops in (None, 0, 1, 2):
                got = ref_hop_distance(n, s, t, sources, dir, max_hops)
                assert got.tolist() == brute_bfs(n, s, t, sources, dir, max_hops), (dir, sources, max_hops)
        rows = ref_hop_distance(n, s, t, [6, 1, 6], dir, None, separate=True)
        assert rows.shape == (3, n) and [r.tolist() for r in rows] == [brute_bfs(n, s, t, [v], dir, None) for v in (6, 1, 6)]
    assert ref_hop_distance(n, s, t, [6], "out").tolist() == [2, -1, -1, 1, -1, -1, 0, -1]
    assert ref_hop_distance(n, s, t, [6], "in").tolist() == [-1, -1, -1, -1, -1, 1, 0, -1]
    assert ref_hop_distance(n, s, t, [], "out", separate=True).shape == (0, n)


def test_restatements_agree_with_scipy():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    for n, e, seed in ((8, None, 0), (300, 257, 1), (300, 1000, 2), (2, 1, 3)):
        s, t = (np.asarray(EIGHT_S), np.asarray(EIGHT_T)) if e is None else random_edges(n, e, seed)
        a = sparse.csr_matrix((np.ones(len(s)), (s, t)), shape=(n, n))
        count, lab = csgraph.connected_components(a, directed=True, connection="weak")
        labels, _ = ref_components(n, s, t)
        rank, k, _, _, _ = ref_rank(labels)
        assert k == count
        assert len(set(zip(lab.tolist(), rank.tolist()))) == count          # the two labellings name the same partition
        src = [0, n - 1, n // 2]
        for dir, m in (("out", a), ("in", a.T), ("both", a + a.T)):
            want = csgraph.shortest_path(sparse.csr_matrix(m), unweighted=True, indices=src)
            want = np.where(np.isinf(want), -1, want).astype(np.int64)
            assert np.array_equal(ref_hop_distance(n, s, t, src, dir, separate=True), want), dir
            assert np.array_equal(ref_hop_distance(n, s, t, src, dir), np.where((want < 0).all(0), -1, np.where(want < 0, n, want).min(0)))


def test_restated_round_counts_on_the_paths():
    """what the GPU file's bound of 64 rounds stands on: the synchronous restatement takes 2 rounds on a sequentially numbered path of
    4096 nodes, forwards or reversed, 3 on the zigzag numbering and at most 10 on random numberings, where neighbour-to-neighbour
    propagation would need up to 4095"""
    n = 4096
    seq = np.arange(n)
    assert ref_components(n, *path_edges(seq))[1] == 2
    assert ref_components(n, *path_edges(seq[::-1]))[1] == 2
    zigzag = np.empty(n, np.int64)
    zigzag[0::2], zigzag[1::2] = np.arange(n // 2), n - 1 - np.arange(n // 2)
    assert ref_components(n, *path_edges(zigzag))[1] == 3
    for k in range(20):
        labels, rounds = ref_components(n, *path_edges(np.random.default_rng(k).permutation(n)))
        assert rounds <= 10 and not labels.any(), k


# ---- names and argument errors ----------------------------------------------------------------------------------------------------

def graph(**kw):
    return ng.GNNGraph([0, 0, 1, 2], [1, 2, 0, 0], num_nodes=3, index_base=0, **kw)


def test_names_are_exported():
    for name in NAMES:
        assert name in ng.__all__, name
        assert callable(getattr(ng, name)), name


def test_entries_are_declared_bound_and_cited():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ngpde.h")).read()
    block = header[header.index("graph traversal on a device COO list"):header.index("GNOConv message (src/layers.jl:527-530)")]
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name + "(" in block, name
    assert block.count("src/NeuralGraphPDE.jl:4") >= 6 and block.count(":16") >= 6          # the block and each entry's comment cite both
    assert "NGPDE_HOP_WAVE_ROW 64" in block and "stale reads" in block and "atomicMin" in block
    makefile = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neuralgraphpde.jl_amd", "csrc", "Makefile")).read()
    assert "coo_rows.h" in makefile and "coo_compact.h" in makefile and "device_scratch.h" in makefile          # what the new file includes
    assert "traverse_rounds.h" in makefile.split("HDRS :=")[1].split("\n")[0]


def test_argument_errors_come_before_any_device_call():
    g = graph()
    for bad in ("BOTH", "sideways", 0, None, True):
        with pytest.raises(ng.ArgumentError, match="dir must be"):
            ng.hop_distance(g, [0], dir=bad)
        with pytest.raises(ng.ArgumentError, match="dir must be"):
            ng.neighborhood(g, [0], 1, dir=bad)
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(ng.ArgumentError, match="max_hops"):
            ng.hop_distance(g, [0], max_hops=bad)
    for bad in (-1, 1.5, "2", True, None):
        with pytest.raises(ng.ArgumentError, match="d must be"):
            ng.neighborhood(g, [0], bad)
    for bad in ([0.5], [True], "0", None, np.array([1.0]), [[0, "a"]]):
        with pytest.raises(ng.ArgumentError, match="integers"):
            ng.hop_distance(g, bad)
        with pytest.raises(ng.ArgumentError, match="integers"):
            ng.neighborhood(g, bad, 1)
    with pytest.raises(ng.ArgumentError, match="separate"):
        ng.hop_distance(g, [0], separate=1)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ng.ArgumentError, match="check_every"):
            ng.hop_distance(g, [0], check_every=bad)
        with pytest.raises(ng.ArgumentError, match="check_every"):
            ng.connected_components(g, check_every=bad)
    with pytest.raises(ng.ArgumentError, match="max_hops must be given"):
        ng.hop_distance(g, [0], check_every=0)
    with pytest.raises(ng.ArgumentError, match="max_rounds must be given"):
        ng.connected_components(g, check_every=0)
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ng.ArgumentError, match="max_rounds"):
            ng.connected_components(g, max_rounds=bad)
    with pytest.raises(ng.ArgumentError, match="no nodes"):
        ng.is_connected(ng.GNNGraph([], [], num_nodes=0, index_base=0))
    with pytest.raises(ng.ArgumentError, match="graph 1 of the batch has no nodes"):
        ng.is_connected(ng.GNNGraph([0], [1], num_nodes=3, index_base=0, graph_indicator=[0, 0, 2], num_graphs=3))


# ---- the C entries --------------------------------------------------------------------------------------------------------------

ONE = C.c_void_p(16)     # (never dereferenced: the checks come before any device call)


def test_workspace_bytes_are_the_formulas_of_the_header():
    """include/ngpde.h, written out: components 256 (the control block); hop distances 3 * (8 n rounded up to 256) + 256; shortest
    paths (2 x 4 n width + 4 nnz_a + 4 nnz_b, each term rounded up to 256) + 256 with width = 1 for one row of dist_out, else
    min(n_sources, NGPDE_SSSP_PASS = 64) rounded up to a multiple of NGPDE_SSSP_LANE_SOURCES = 4; 0 for the sizes they refuse"""
    lib = _lib.load()
    up = lambda x: (x + 255) // 256 * 256
    refused = (-1, 2 ** 31)
    for n in (0, 1, 31, 32, 33):
        assert lib.ngpde_coo_components_workspace_bytes(n) == 256
        assert lib.ngpde_csr_hop_distance_workspace_bytes(n) == 3 * up(8 * n) + 256
        for nnz in (0, 1, 64):
            for k in (0, 1, 4, 5, 64, 65):
                for separate in (0, 1):
                    width = 1 if not separate or min(k, 64) <= 1 else (min(k, 64) + 3) // 4 * 4
                    want = 2 * up(4 * n * width) + up(4 * nnz) + up(4 * nnz) + 256
                    assert lib.ngpde_csr_shortest_paths_workspace_bytes(n, nnz, nnz, k, separate) == want, (n, nnz, k, separate)
                    assert lib.ngpde_csr_shortest_paths_workspace_bytes(n, nnz, 0, k, separate) == want - up(4 * nnz), (n, nnz, k, separate)
    for bad in refused:
        assert lib.ngpde_coo_components_workspace_bytes(bad) == 0 and lib.ngpde_csr_hop_distance_workspace_bytes(bad) == 0
        for separate in (0, 1):
            for at in range(4):
                sizes = [33, 64, 64, 5]
                sizes[at] = bad
                assert lib.ngpde_csr_shortest_paths_workspace_bytes(*sizes, separate) == 0, (sizes, separate)


def test_components_entries_refuse_null_and_negative_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT

    def label(n=3, e=4, s=ONE, t=ONE, max_rounds=0, check_every=4, labels=ONE, rounds=ONE, ws=ONE, ws_bytes=256):
        return lib.ngpde_coo_components(n, e, s, t, 0, max_rounds, check_every, labels, rounds, ws, ws_bytes, None)

    def rank(n=3, labels=ONE, n_graphs=1, graph_of=None, outs=(ONE, ONE, ONE, ONE), count=True, per_graph=None):
        n64 = C.c_int64(7)
        return lib.ngpde_components_rank(n, labels, n_graphs, graph_of, *outs, C.byref(n64) if count else None, per_graph, None), n64.value

    for n, e in ((-1, 0), (3, -1)):
        assert label(n, e) == bad and b"negative" in lib.ngpde_last_error()
    for n, e in ((2 ** 31, 1), (3, 2 ** 31)):
        assert label(n, e) == bad and b"2^31" in lib.ngpde_last_error()
    for kw in (dict(s=None), dict(t=None), dict(labels=None)):
        assert label(**kw) == bad and b"NULL" in lib.ngpde_last_error(), kw
    assert label(n=0) == _lib.ERR_DIMENSION_MISMATCH
    assert label(max_rounds=-1) == bad and b"max_rounds" in lib.ngpde_last_error()
    assert label(check_every=-1) == bad and b"check_every" in lib.ngpde_last_error()
    assert label(ws=None) == _lib.ERR_WORKSPACE
    assert label(ws_bytes=255) == _lib.ERR_WORKSPACE and b"needed" in lib.ngpde_last_error()
    assert label(ws=C.c_void_p(20)) == bad and b"aligned" in lib.ngpde_last_error()
    assert label(max_rounds=2 ** 31 - 1, check_every=0) == _lib.ERR_UNSUPPORTED and b"launches" in lib.ngpde_last_error()
    size = lib.ngpde_coo_components_workspace_bytes
    assert [size(n) for n in (0, 1, 4096, 2 ** 31 - 1)] == [256] * 4 and size(-1) == 0 and size(2 ** 31) == 0

    assert rank(count=False)[0] == bad and b"count_out is NULL" in lib.ngpde_last_error()
    assert rank(n=-1) == (bad, 0) and b"negative" in lib.ngpde_last_error()
    assert rank(n=2 ** 31 - 1) == (bad, 0) and b"2^31" in lib.ngpde_last_error()
    assert rank(n_graphs=0) == (bad, 0) and b"n_graphs" in lib.ngpde_last_error()
    assert rank(n_graphs=2) == (bad, 0) and b"graph_of is NULL" in lib.ngpde_last_error()
    assert rank(labels=None) == (bad, 0) and b"NULL" in lib.ngpde_last_error()
    for k in range(4):
        outs = [ONE] * 4
        outs[k] = None
        assert rank(outs=tuple(outs)) == (bad, 0) and b"NULL" in lib.ngpde_last_error(), k


def test_rows_and_hop_entries_refuse_null_and_negative_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT

    def rows(n=3, e=4, s=ONE, t=ONE, dir=0, outs=(ONE, ONE)):
        return lib.ngpde_coo_rows(n, e, s, t, 0, dir, *outs, None)

    def hop(n=3, a=(4, ONE, ONE), b=(0, None, None), k=2, sources=ONE, separate=0, max_hops=-1, check_every=8, dist=ONE, ws=ONE,
            ws_bytes=1 << 20):
        return lib.ngpde_csr_hop_distance(n, *a, *b, k, sources, 0, separate, max_hops, check_every, dist, ws, ws_bytes, None)

    def reached(n=3, dist=ONE, nodes=ONE, out=True):
        n64 = C.c_int64(7)
        return lib.ngpde_hop_reached_nodes(n, dist, 0, nodes, C.byref(n64) if out else None, None), n64.value

    for n, e in ((-1, 0), (3, -1)):
        assert rows(n, e) == bad and b"negative" in lib.ngpde_last_error()
    for n, e in ((2 ** 31, 1), (3, 2 ** 31)):
        assert rows(n, e) == bad and b"2^31" in lib.ngpde_last_error()
    for dir in (-1, 2):
        assert rows(dir=dir) == bad and b"dir" in lib.ngpde_last_error()
    for kw in (dict(s=None), dict(t=None), dict(outs=(None, ONE)), dict(outs=(ONE, None))):
        assert rows(**kw) == bad and b"NULL" in lib.ngpde_last_error(), kw
    assert rows(n=0) == _lib.ERR_DIMENSION_MISMATCH

    for kw in (dict(n=-1), dict(k=-1)):
        assert hop(**kw) == bad and b"negative" in lib.ngpde_last_error()
    for kw in (dict(n=2 ** 31), dict(k=2 ** 31)):
        assert hop(**kw) == bad and b"2^31" in lib.ngpde_last_error()
    for a in ((-1, ONE, ONE), (2 ** 31, ONE, ONE)):
        assert hop(a=a) == bad and b"nnz_a" in lib.ngpde_last_error()
    for a in ((4, None, ONE), (4, ONE, None)):
        assert hop(a=a) == bad and b"NULL" in lib.ngpde_last_error()
    for b in ((-1, ONE, ONE), (4, None, ONE), (4, ONE, None)):
        assert hop(b=b) == bad, b
    assert hop(sources=None) == bad and b"sources is NULL" in lib.ngpde_last_error()
    assert hop(check_every=-1) == bad and b"check_every" in lib.ngpde_last_error()
    assert hop(check_every=0) == bad and b"max_hops" in lib.ngpde_last_error()
    assert hop(dist=None) == bad and b"dist_out is NULL" in lib.ngpde_last_error()
    assert hop(ws=None) == _lib.ERR_WORKSPACE
    size = lib.ngpde_csr_hop_distance_workspace_bytes
    assert hop(ws_bytes=size(3) - 1) == _lib.ERR_WORKSPACE and b"needed" in lib.ngpde_last_error()
    assert hop(k=2 ** 20, separate=1, n=2 ** 21) == _lib.ERR_UNSUPPORTED and b"too large" in lib.ngpde_last_error()
    assert hop(check_every=0, max_hops=2 ** 40, n=2 ** 30, ws_bytes=1 << 40) == _lib.ERR_UNSUPPORTED and b"launches" in lib.ngpde_last_error()
    assert hop(n=0, k=0, sources=None, dist=None, ws=None) == 0 and hop(k=0, separate=1, sources=None, dist=None, ws=None) == 0      # nothing to write
    # the header's formula: seen and the two frontiers, 8 n bytes each rounded up to 256, and the control block
    for n in (0, 1, 31, 32, 33, 300, 16384, 100003):
        assert size(n) == 3 * ((8 * n + 255) // 256 * 256) + 256, n
    assert size(-1) == 0 and size(2 ** 31) == 0

    assert reached(out=False)[0] == bad and b"n_out is NULL" in lib.ngpde_last_error()
    assert reached(n=-1) == (bad, 0) and b"negative" in lib.ngpde_last_error()
    assert reached(n=2 ** 31) == (bad, 0) and b"2^31" in lib.ngpde_last_error()
    for kw in (dict(dist=None), dict(nodes=None)):
        assert reached(**kw) == (bad, 0) and b"NULL" in lib.ngpde_last_error()
    assert reached(n=0, dist=None, nodes=None) == (0, 0)
