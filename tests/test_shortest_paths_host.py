"""Host-side checks of the weighted shortest paths (traversal.shortest_paths over csrc/graph_paths.hip; the reference's GNNGraph is a
Graphs.AbstractGraph, src/NeuralGraphPDE.jl:4 / :16, so dijkstra_shortest_paths and bellman_ford_shortest_paths work on it): the numpy
float32 restatement of the double-buffered rounds that tests/test_shortest_paths_gpu.py compares the device with BITWISE, pinned here
against an independent float32 heapq Dijkstra (bitwise), against scipy.sparse.csgraph.dijkstra in float64 (a derived bound) and by the
tree and tightness of its parents; the exported names, the entries of the C ABI, and the argument errors raised before any device call.
No GPU."""
import ctypes as C
import functools
import heapq
import os

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib
from test_traversal_host import random_edges

NAMES = ("ShortestPaths", "shortest_paths")
ENTRIES = ("ngpde_coo_rows_eid", "ngpde_csr_shortest_paths_workspace_bytes", "ngpde_csr_shortest_paths")
FAMILIES = ("uniform", "ties", "magnitudes", "inf")
INF = np.float32(np.inf)


# ---- the numpy restatement (the yardstick of the GPU file) ----------------------------------------------------------------------

def weights(family, e, seed):
    """the four weight families, float32[e]"""
    rng = np.random.default_rng(seed)
    if family == "uniform":
        w = rng.uniform(0.5, 1.5, e)
    elif family == "ties":                                       # small integers: many equal path lengths, and zeros
        w = rng.integers(0, 4, e)
    elif family == "magnitudes":                                 # 1e-9 .. 1e2: small weights are absorbed by large distances
        w = 10.0 ** rng.uniform(-9, 2, e)
    elif family == "inf":
        w = np.array([0.0, 1.0, 2.0, np.inf])[rng.integers(0, 4, e)]
    else:
        raise ValueError(family)
    return w.astype(np.float32)


def row_order(n, s, t, dir):
    """(row_ptr, other, eid): the entries of every node's row in ROW ORDER -- COO order inside a row; for dir="both" the entries
    grouped by target (the edges into the node) before those grouped by source.  Following s -> t a node is relaxed from the sources
    of its incoming edges."""
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    pos = np.arange(len(s), dtype=np.int64)
    sets = {"out": [(t, s)], "in": [(s, t)], "both": [(t, s), (s, t)]}[dir]
    row = np.concatenate([a for a, _ in sets])
    other = np.concatenate([b for _, b in sets])
    eid = np.concatenate([pos] * len(sets))
    which = np.concatenate([np.full(len(s), k) for k in range(len(sets))])
    order = np.lexsort((eid, which, row))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))])
    return ptr, other[order], eid[order]


def ref_shortest_paths(n, s, t, w, sources, dir="out", max_dist=None, separate=False):
    """(dist float32, parent_eid int32, parents int32, rounds): the double-buffered rounds.  A round reads the distances of the round
    before only: best[v] = the smallest fl32(d[other] + w) over v's row (candidates above max_dist dropped); where best[v] < d[v]
    STRICTLY the node takes it and records the FIRST entry of its row that attains it.  The first round that lowers nothing ends it
    and counts: `rounds` includes the confirming round; no sources, no rounds.  separate: one row per listed source, rounds the
    largest of theirs."""
    sources = np.asarray(sources, np.int64).reshape(-1)
    w = np.ones(len(s), np.float32) if w is None else np.asarray(w, np.float32)
    if separate:
        out = [ref_shortest_paths(n, s, t, w, [v], dir, max_dist) for v in sources]
        if not out:
            return np.zeros((0, n), np.float32), np.zeros((0, n), np.int32), np.zeros((0, n), np.int32), 0
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]), max(o[3] for o in out)
    ptr, other, eid = row_order(n, s, t, dir)
    w_rows = w[eid]
    row = np.repeat(np.arange(n), np.diff(ptr))
    filled = np.flatnonzero(np.diff(ptr))
    limit = INF if max_dist is None else np.float32(max_dist)
    dist = np.full(n, INF)
    dist[sources] = 0
    parent_eid, parents = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    rounds = 0
    while len(sources):
        rounds += 1
        cand = dist[other] + w_rows                                  # float32 + float32: ONE rounding, as on the device
        assert cand.dtype == np.float32
        cand[~(cand <= limit)] = INF
        best = np.full(n, INF)
        if len(filled):
            best[filled] = np.minimum.reduceat(cand, ptr[filled])
        lowered = best < dist
        if not lowered.any():
            break
        first = np.flatnonzero((cand == best[row]) & lowered[row])
        nodes, at = np.unique(row[first], return_index=True)          # the rows are contiguous: the first hit of every lowered row
        parent_eid[nodes], parents[nodes] = eid[first[at]], other[first[at]]
        dist = np.where(lowered, best, dist)
    return dist, parent_eid, parents, rounds


# ---- the independent yardsticks -----------------------------------------------------------------------------------------------------

def heap_dijkstra(n, s, t, w, sources, dir="out", max_dist=None):
    """a textbook float32 Dijkstra on a binary heap: every sum is rounded to float32"""
    nbrs = [[] for _ in range(n)]
    for a, b, x in zip(s, t, w):
        if dir in ("out", "both"):
            nbrs[a].append((b, np.float32(x)))
        if dir in ("in", "both"):
            nbrs[b].append((a, np.float32(x)))
    dist = [INF] * n
    heap = []
    for v in sources:
        dist[v] = np.float32(0)
        heap.append((np.float32(0), int(v)))
    heapq.heapify(heap)
    done = [False] * n
    while heap:
        d, v = heapq.heappop(heap)
        if done[v]:
            continue
        done[v] = True
        for u, x in nbrs[v]:
            c = np.float32(d + x)
            if c < dist[u] and (max_dist is None or c <= np.float32(max_dist)):
                dist[u] = c
                heapq.heappush(heap, (c, u))
    return np.array(dist, np.float32)


def check_tree_and_tight(n, s, t, w, sources, dist, parent_eid, parents, dir):
    """the parents form a tree rooted at the sources, every parent edge is an edge of the graph INTO the node (for this dir) and is
    tight: fl32(d[parent] + w) == d[v]"""
    s, t, w = np.asarray(s, np.int64), np.asarray(t, np.int64), np.asarray(w, np.float32)
    has = parent_eid >= 0
    assert np.array_equal(has, parents >= 0)
    is_source = np.zeros(n, bool)
    is_source[np.asarray(sources, np.int64)] = True
    assert np.array_equal(has, np.isfinite(dist) & ~is_source)              # -1 exactly at the sources and the unreached nodes
    v = np.flatnonzero(has)
    e, p = parent_eid[v], parents[v].astype(np.int64)
    into = {"out": (t[e] == v) & (s[e] == p), "in": (s[e] == v) & (t[e] == p)}
    into["both"] = into["out"] | into["in"]
    assert into[dir].all()
    assert np.array_equal(dist[p] + w[e], dist[v])                          # tight, in float32
    at = np.arange(n)                                                       # acyclic: every chain ends at a source within n links
    for _ in range(n):
        step = parents[at] >= 0
        if not step.any():
            break
        at = np.where(step, parents[at], at)
    assert (parents[at] < 0).all() and (is_source[at] | ~has).all()


@functools.lru_cache(maxsize=None)
def random_case(k):
    """graph k of the 60: N < 300, E < 1500, one of the four families"""
    rng = np.random.default_rng(9000 + k)
    n, e = int(rng.integers(1, 300)), int(rng.integers(0, 1500))
    s, t = random_edges(n, e, 77 + k) if e else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    sources = rng.integers(0, n, int(rng.integers(1, 4)))
    return n, s, t, weights(FAMILIES[k % 4], e, k), sources, ("out", "in", "both")[k % 3]


def test_restatement_is_bitwise_a_float32_heap_dijkstra():
    for k in range(60):
        n, s, t, w, sources, dir = random_case(k)
        dist, parent_eid, parents, rounds = ref_shortest_paths(n, s, t, w, sources, dir)
        want = heap_dijkstra(n, s, t, w, sources, dir)
        assert dist.dtype == np.float32 and dist.tobytes() == want.tobytes(), k
        assert 1 <= rounds <= n, k                                          # N rounds always suffice, the confirming one included
        check_tree_and_tight(n, s, t, w, sources, dist, parent_eid, parents, dir)
        finite = np.sort(dist[np.isfinite(dist)])
        cut = finite[len(finite) // 2]                                      # a distance that occurs: the boundary of max_dist
        near, pe, pa, _ = ref_shortest_paths(n, s, t, w, sources, dir, max_dist=cut)
        assert near.tobytes() == np.where(dist <= cut, dist, INF).tobytes(), k
        assert near.tobytes() == heap_dijkstra(n, s, t, w, sources, dir, max_dist=cut).tobytes(), k
        check_tree_and_tight(n, s, t, w, sources, near, pe, pa, dir)


def test_restatement_agrees_with_scipy_float64_within_the_rounding_bound():
    """each float32 add errs by at most 2^-24 relative and all terms are non-negative, so a path of k edges is off by at most
    (1 + 2^-24)^k - 1 relative, either way; a shortest path found in `rounds` rounds has fewer than `rounds` edges"""
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    for k in range(60):
        n, s, t, w, sources, dir = random_case(k)
        dist, _, _, rounds = ref_shortest_paths(n, s, t, w, sources, dir, separate=True)
        keep = np.isfinite(w)                                               # an edge of length +inf reaches nothing
        a, b, x = s[keep], t[keep], w[keep].astype(np.float64)
        if dir == "in":
            a, b = b, a
        elif dir == "both":
            a, b, x = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([x, x])
        order = np.lexsort((x, b, a))                                       # parallel edges: the shortest of each pair (a, b)
        a, b, x = a[order], b[order], x[order]
        head = np.ones(len(a), bool)
        head[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
        m = sparse.csr_matrix((x[head], (a[head], b[head])), shape=(n, n))  # explicit zeros stay: edges of length 0
        want = csgraph.dijkstra(m, directed=True, indices=sources)
        assert np.array_equal(np.isfinite(dist), np.isfinite(want)), k
        ok = np.isfinite(want)
        bound = ((1.0 + 2.0 ** -24) ** rounds - 1.0) * want[ok]
        err = np.abs(dist[ok].astype(np.float64) - want[ok])
        assert (err <= bound).all(), (k, float((err - bound).max()))


def test_restatement_on_hand_written_graphs():
    # 0 -> 1 -> 2 and a direct edge 0 -> 2 of the same length: node 2 is first reached by the direct edge (round 1) and keeps it
    s, t, w = [0, 1, 0], [1, 2, 2], np.float32([1, 1, 2])
    dist, pe, pa, rounds = ref_shortest_paths(3, s, t, w, [0])
    assert dist.tolist() == [0, 1, 2] and pe.tolist() == [-1, 0, 2] and pa.tolist() == [-1, 0, 0] and rounds == 2
    # ... and takes the two-edge path only if it is STRICTLY shorter
    dist, pe, pa, rounds = ref_shortest_paths(3, s, t, np.float32([1, 0.5, 2]), [0])
    assert dist.tolist() == [0, 1, 1.5] and pe.tolist() == [-1, 0, 1] and pa.tolist() == [-1, 0, 1] and rounds == 3
    # two equal candidates in ONE round: the first in row order (the smaller COO position) wins; permuting the list changes it
    dist, pe, pa, _ = ref_shortest_paths(3, [1, 0], [2, 2], np.float32([1, 1]), [0, 1])
    assert dist.tolist() == [0, 0, 1] and pe.tolist() == [-1, -1, 0] and pa.tolist() == [-1, -1, 1]
    # dir="both": the edges into the node come before the edges out of it
    dist, pe, pa, _ = ref_shortest_paths(3, [2, 0], [1, 2], np.float32([1, 1]), [0, 1], "both")
    assert dist.tolist() == [0, 0, 1] and pe.tolist() == [-1, -1, 1] and pa.tolist() == [-1, -1, 0]
    # a zero-weight cycle cannot make a parent cycle; absorption: 1e-9 vanishes beside 100
    dist, pe, pa, _ = ref_shortest_paths(3, [0, 1, 2], [1, 2, 1], np.float32([100, 0, 0]), [0])
    assert dist.tolist() == [0, 100, 100] and pa.tolist() == [-1, 0, 1]
    dist, _, _, _ = ref_shortest_paths(3, [0, 1], [1, 2], np.float32([100, 1e-9]), [0])
    assert dist[2] == np.float32(100)
    # no sources, no edges, separate
    dist, pe, pa, rounds = ref_shortest_paths(3, s, t, w, [])
    assert np.isinf(dist).all() and (pe == -1).all() and rounds == 0
    assert ref_shortest_paths(2, [], [], None, [1])[0].tolist() == [np.inf, 0] and ref_shortest_paths(2, [], [], None, [1])[3] == 1
    rows = ref_shortest_paths(3, s, t, w, [2, 0, 2], separate=True)
    assert rows[0].shape == (3, 3) and rows[0][1].tolist() == [0, 1, 2] and rows[0][0].tolist() == [np.inf, np.inf, 0] and rows[3] == 2
    assert ref_shortest_paths(3, s, t, w, [], separate=True)[0].shape == (0, 3)
    # unit weights are hop distances
    assert ref_shortest_paths(3, s, t, None, [0])[0].tolist() == [0, 1, 1]


# ---- names, entries and argument errors -------------------------------------------------------------------------------------------

def graph(**kw):
    return ng.GNNGraph([0, 0, 1, 2], [1, 2, 0, 0], num_nodes=3, index_base=0, **kw)


def test_names_are_exported():
    for name in NAMES:
        assert name in ng.__all__ and name in ng.traversal.__all__, name
        assert callable(getattr(ng, name)), name
    assert (_lib.SSSP_WAVE_ROW, _lib.SSSP_PASS, _lib.SSSP_LANE_SOURCES) == (64, 64, 4)
    assert "gradient" in ng.shortest_paths.__doc__


def test_entries_are_declared_bound_and_cited():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ngpde.h")).read()
    block = header[header.index("graph traversal on a device COO list"):header.index("GNOConv message (src/layers.jl:527-530)")]
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name + "(" in block, name
    new = block[block.index("The rows plan with its COO positions"):]
    assert new.count("src/NeuralGraphPDE.jl:4, :16") == 2                     # each entry's comment cites both lines
    for text in ("#define NGPDE_SSSP_WAVE_ROW 64", "#define NGPDE_SSSP_PASS 64", "#define NGPDE_SSSP_LANE_SOURCES 4", "DOUBLE-BUFFERED",
                 "STRICTLY decreases", "no atomics", "FIXED POINT"):
        assert text in new, text
    source = open(os.path.join(root, "neuralgraphpde.jl_amd", "csrc", "graph_paths.hip")).read()
    assert "__launch_bounds__(256)" in source and "atomic" not in source.split("namespace ngpde {")[1].replace("report_offender", "")
    shared = open(os.path.join(root, "neuralgraphpde.jl_amd", "csrc", "traverse_rounds.h")).read()          # what the round kernel includes
    assert '#include "traverse_rounds.h"' in source and "atomic" not in shared.split("namespace ngpde {")[1].replace("report_offender", "")


def test_argument_errors_come_before_any_device_call():
    g = graph()
    for bad in ("BOTH", "sideways", 0, None, True):
        with pytest.raises(ng.ArgumentError, match="dir must be"):
            ng.shortest_paths(g, [0], dir=bad)
    for bad in ([0.5], [True], "0", None, np.array([1.0])):
        with pytest.raises(ng.ArgumentError, match="integers"):
            ng.shortest_paths(g, bad)
    for name in ("separate", "return_parents"):
        with pytest.raises(ng.ArgumentError, match=name):
            ng.shortest_paths(g, [0], **{name: 1})
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ng.ArgumentError, match="check_every"):
            ng.shortest_paths(g, [0], check_every=bad)
    with pytest.raises(ng.ArgumentError, match="max_rounds must be given"):
        ng.shortest_paths(g, [0], check_every=0)
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ng.ArgumentError, match="max_rounds"):
            ng.shortest_paths(g, [0], max_rounds=bad)
    for bad in (-1, -0.5, float("nan"), "2", True):
        with pytest.raises(ng.ArgumentError, match="max_dist"):
            ng.shortest_paths(g, [0], max_dist=bad)
    for bad in (np.ones(4), np.ones(4, np.int32), [1, 1, 1, 1]):
        with pytest.raises(ng.ArgumentError, match="float32"):
            ng.shortest_paths(g, [0], edge_weight=bad)
    with pytest.raises(ng.DimensionMismatch, match="3 entries for 4 edges"):
        ng.shortest_paths(g, [0], edge_weight=np.ones(3, np.float32))
    sp = ng.ShortestPaths(np.zeros(3, np.float32), None, None, np.zeros(2, np.int32))
    with pytest.raises(ng.ArgumentError, match="return_parents=True"):
        sp.path_to(0)


ONE = C.c_void_p(16)     # (never dereferenced: the checks come before any device call)


def test_entries_refuse_null_and_negative_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    size = lib.ngpde_csr_shortest_paths_workspace_bytes

    def rows(n=3, e=4, s=ONE, t=ONE, dir=0, outs=(ONE, ONE, ONE)):
        return lib.ngpde_coo_rows_eid(n, e, s, t, 0, dir, *outs, None)

    def paths(n=3, a=(4, ONE, ONE, ONE), b=(0, None, None, None), k=2, sources=ONE, separate=0, weights=ONE, max_dist=np.inf, max_rounds=0,
              check_every=8, dist=ONE, parent_eid=None, parent=None, rounds=None, ws=ONE, ws_bytes=1 << 20):
        return lib.ngpde_csr_shortest_paths(n, *a, *b, k, sources, 0, separate, weights, max_dist, max_rounds, check_every, dist, parent_eid,
                                            parent, rounds, ws, ws_bytes, None)

    for n, e in ((-1, 0), (3, -1)):
        assert rows(n, e) == bad and b"negative" in lib.ngpde_last_error()
    for n, e in ((2 ** 31, 1), (3, 2 ** 31)):
        assert rows(n, e) == bad and b"2^31" in lib.ngpde_last_error()
    for dir in (-1, 2):
        assert rows(dir=dir) == bad and b"dir" in lib.ngpde_last_error()
    for kw in (dict(s=None), dict(t=None), dict(outs=(None, ONE, ONE)), dict(outs=(ONE, None, ONE)), dict(outs=(ONE, ONE, None))):
        assert rows(**kw) == bad and b"NULL" in lib.ngpde_last_error(), kw
    assert rows(n=0) == _lib.ERR_DIMENSION_MISMATCH

    for kw in (dict(n=-1), dict(k=-1), dict(a=(-1, ONE, ONE, ONE)), dict(b=(-1, ONE, ONE, ONE))):
        assert paths(**kw) == bad and b"negative" in lib.ngpde_last_error(), kw
    for kw in (dict(n=2 ** 31), dict(k=2 ** 31), dict(a=(2 ** 31, ONE, ONE, ONE))):
        assert paths(**kw) == bad and b"2^31" in lib.ngpde_last_error(), kw
    for a in ((4, None, ONE, ONE), (4, ONE, None, ONE), (4, ONE, ONE, None)):
        assert paths(a=a) == bad and b"set a is NULL" in lib.ngpde_last_error()
    for b in ((4, None, ONE, ONE), (4, ONE, None, ONE), (4, ONE, ONE, None)):
        assert paths(b=b) == bad and b"set b is NULL" in lib.ngpde_last_error()
    assert paths(b=(5, ONE, ONE, ONE)) == bad and b"ONE list" in lib.ngpde_last_error()
    assert paths(sources=None) == bad and b"sources is NULL" in lib.ngpde_last_error()
    for v in (-1.0, np.nan):
        assert paths(max_dist=v) == bad and b"max_dist" in lib.ngpde_last_error()
    assert paths(max_rounds=-1) == bad and b"max_rounds" in lib.ngpde_last_error()
    assert paths(check_every=-1) == bad and b"check_every" in lib.ngpde_last_error()
    assert paths(check_every=0) == bad and b"max_rounds must be given" in lib.ngpde_last_error()
    assert paths(dist=None) == bad and b"dist_out is NULL" in lib.ngpde_last_error()
    assert paths(ws=None) == _lib.ERR_WORKSPACE
    assert paths(ws_bytes=size(3, 4, 0, 2, 0) - 1) == _lib.ERR_WORKSPACE and b"needed" in lib.ngpde_last_error()
    assert paths(ws=C.c_void_p(20)) == bad and b"aligned" in lib.ngpde_last_error()
    assert paths(k=2 ** 20, separate=1, n=2 ** 21, ws_bytes=1 << 50) == _lib.ERR_UNSUPPORTED and b"too large" in lib.ngpde_last_error()
    assert paths(check_every=0, max_rounds=2 ** 21) == _lib.ERR_UNSUPPORTED and b"launches" in lib.ngpde_last_error()
    # the header's formula: the two round buffers of a pass, the weights of both sets in row order, and the control block
    up = lambda x: (x + 255) // 256 * 256
    for n, ea, eb, k, separate in ((0, 0, 0, 0, 0), (1, 0, 0, 1, 0), (300, 1000, 0, 5, 0), (300, 1000, 1000, 5, 1), (300, 257, 257, 63, 1),
                                   (300, 257, 0, 64, 1), (300, 257, 0, 65, 1), (100003, 1000, 1000, 130, 1), (7, 3, 3, 0, 1), (7, 3, 3, 1, 1)):
        rows_here = min(k, _lib.SSSP_PASS) if separate else 1
        width = 1 if rows_here <= 1 else (rows_here + _lib.SSSP_LANE_SOURCES - 1) // _lib.SSSP_LANE_SOURCES * _lib.SSSP_LANE_SOURCES
        assert size(n, ea, eb, k, separate) == 2 * up(4 * n * width) + up(4 * ea) + up(4 * eb) + 256, (n, ea, eb, k, separate)
    assert size(-1, 0, 0, 0, 0) == 0 and size(2 ** 31, 0, 0, 0, 0) == 0 and size(3, -1, 0, 0, 0) == 0 and size(3, 0, 0, 2 ** 31, 1) == 0
