"""GPU tests of the queries by node and by pair (queries.py over csrc/graph_query.hip; src/NeuralGraphPDE.jl:4 of the reference re-exports
has_edge, neighbors / inneighbors / outneighbors, adjacency_list, intersect and random_walk_pe with GNNGraphs).

Every reference is a numpy restatement, written in tests/test_graph_queries_host.py (where brute-force loops pin it without a GPU) and
imported here.  Structure and order are compared exactly; the only values under a tolerance are random_walk_pe's, and that bound is
derived: with u2 = 2^-23 and m the longest row of A, one step's entry is a sum of at most m products of a once-rounded RW entry, so
to first order |pe - ref|[k - 1][i] <= k * (m + 3) * u2 * (|RW|^k)[i][i], |RW| built from |A[i][j]| * |inv[j]|.
"""
import functools
import gc

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib
from test_graph_queries_host import random_edges, ref_adjacency, ref_has_edge, ref_intersect, ref_random_walk

pytestmark = pytest.mark.gpu
DEV = "cuda"

BIG = 100003
SIZES = [(n, e) for n in (1, 2, 300) for e in (0, 1, 255, 256, 257, 1000)] + [(BIG, 1000)]          # the last: s * n + t needs 64 bits
LOW32_A, LOW32_B = 5, 7          # at BIG: (a, b) and (a + ds, b + dt) with ds * n + dt = 2^32 share the low 32 bits of their keys


def low32_partner(n):
    ds, dt = divmod(2 ** 32, n)
    return LOW32_A + ds, LOW32_B + dt


@functools.lru_cache(maxsize=None)
def edges(n, e, seed=None):
    s, t = random_edges(n, e, seed=n + e if seed is None else seed)
    if n == BIG:
        a2, b2 = low32_partner(n)
        assert (LOW32_A * n + LOW32_B) % 2 ** 32 == (a2 * n + b2) % 2 ** 32 and a2 < n and b2 < n
        s[10], t[10] = n - 1, n - 1
        s[22], t[22] = LOW32_A, LOW32_B
        s[23], t[23] = a2, b2
    s.flags.writeable = t.flags.writeable = False
    return s, t


def weights(e, seed):
    return (0.5 + np.random.default_rng(seed + 1000).random(e)).astype(np.float32)


def graph(n, s, t, w=None, **kw):
    return ng.GNNGraph(s, t, num_nodes=n, index_base=0, edge_weight=w, **kw)


def host(x):
    return x.detach().cpu().numpy()


def dev64(a):
    return torch.as_tensor(np.asarray(a, np.int64), device=DEV)


# ---- has_edge -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,e", SIZES)
def test_has_edge(n, e):
    s, t = edges(n, e)
    g = graph(n, s, t)
    rng = np.random.default_rng(n + 3 * e)
    qs, qt = np.concatenate([s, rng.integers(0, n, e)]), np.concatenate([t, rng.integers(0, n, e)])
    want_found, want_eid = ref_has_edge(n, s, t, qs, qt)
    found = ng.has_edge(g, dev64(qs), dev64(qt))
    assert found.dtype == torch.bool and found.shape == (2 * e,) and found.is_cuda
    assert np.array_equal(host(found), want_found) and bool(found[:e].all())          # every edge of the graph is found
    plans = [v for k, v in g._shared.items() if k[0] == "keyplan"]
    eid = ng.has_edge(g, qs.tolist(), qt.tolist(), return_eid=True)
    assert eid.dtype == torch.int32 and np.array_equal(host(eid), want_eid)            # the smallest position of a duplicate; -1
    assert len(plans) == 1 and [v for k, v in g._shared.items() if k[0] == "keyplan"][0] is plans[0]          # sorted once
    assert torch.equal(ng.has_edge(g, dev64(qs), dev64(qt)), found)
    none = ng.has_edge(g, dev64([]), dev64([]))
    assert none.dtype == torch.bool and none.numel() == 0
    if e:
        assert ng.has_edge(g, int(s[e // 2]), int(t[e // 2])) is True
        assert ng.has_edge(g, int(s[-1]), int(t[-1]), return_eid=True) == int(want_eid[e - 1])
    if n == BIG:
        a2, b2 = low32_partner(n)
        assert ng.has_edge(g, [LOW32_A, a2, n - 1], [LOW32_B, b2, n - 1], return_eid=True).tolist() == [22, 23, 10]
        assert ng.has_edge(g, LOW32_A + 1, LOW32_B) is False
        g2 = graph(n, np.delete(s, 23), np.delete(t, 23))          # without the partner a 32-bit key would still find it
        assert ng.has_edge(g2, [LOW32_A, a2], [LOW32_B, b2]).tolist() == [True, False]
    for bad_s, bad_t, offender in (([0, n], [0, 0], n), ([0], [n + 5], n + 5), ([-1], [0], -1)):          # an end equal to n is named
        with pytest.raises(ng.DimensionMismatch, match=rf"node {offender}\b"):
            ng.has_edge(g, bad_s, bad_t)
    with pytest.raises(ng.DimensionMismatch, match=rf"node {n}\b"):
        ng.has_edge(g, 0, n)


def test_has_edge_names_the_smallest_offender():
    g = graph(300, *edges(300, 255))
    with pytest.raises(ng.DimensionMismatch, match=r"node -7\b"):
        ng.has_edge(g, [0, 400, 1, -7], [300, 0, 2, 3])
    with pytest.raises(ng.DimensionMismatch, match=r"node 300\b"):
        ng.has_edge(g, [0, 400, 1], [300, 0, 2])


# ---- adjacency_list -------------------------------------------------------------------------------------------------------------

def check_rows(al, n, s, t, nodes, dir):
    ptr, nb, eid = ref_adjacency(n, s, t, nodes, dir)
    assert al.ptr.dtype == al.neighbors.dtype == al.eid.dtype == torch.int32 and al.neighbors.is_cuda
    assert len(al) == len(ptr) - 1
    assert np.array_equal(host(al.ptr), ptr) and np.array_equal(host(al.neighbors), nb) and np.array_equal(host(al.eid), eid)
    own, other = (s, t) if dir == "out" else (t, s)
    listed = np.arange(n) if nodes is None else np.asarray(nodes, np.int64)
    assert np.array_equal(own[host(al.eid)], np.repeat(listed, np.diff(ptr)))          # s[eid], t[eid] reproduce the rows
    assert np.array_equal(other[host(al.eid)], host(al.neighbors))
    return ptr, nb


@pytest.mark.parametrize("dir", ["out", "in"])
@pytest.mark.parametrize("n,e", SIZES)
def test_adjacency_list(n, e, dir):
    s, t = edges(n, e)
    g = graph(n, s, t)
    rng = np.random.default_rng(7 * n + e)
    al = ng.adjacency_list(g, dir=dir)
    ptr, nb = check_rows(al, n, s, t, None, dir)
    assert torch.equal(ng.adjacency_list(g, dir=dir).neighbors, al.neighbors)
    if n <= 300:
        assert al.tolist() == [nb[ptr[i]:ptr[i + 1]].tolist() for i in range(n)]
    subset = rng.permutation(n)[:max(1, n // 3)]
    check_rows(ng.adjacency_list(g, subset, dir), n, s, t, subset, dir)
    repeated = np.concatenate([subset[:5], subset[:2], [n - 1, 0, n - 1]])
    al = ng.adjacency_list(g, dev64(repeated), dir)
    ptr, nb = check_rows(al, n, s, t, repeated, dir)
    for i in (0, len(repeated) - 1):
        assert host(al[i]).tolist() == nb[ptr[i]:ptr[i + 1]].tolist()
    assert torch.equal(al[-1], al[len(repeated) - 1])
    empty = ng.adjacency_list(g, [], dir)
    assert len(empty) == 0 and empty.tolist() == [] and host(empty.ptr).tolist() == [0]
    v = int(subset[0])
    one = ref_adjacency(n, s, t, [v], dir)[1]
    assert host(ng.neighbors(g, v, dir)).tolist() == one.tolist()
    assert host(ng.outneighbors(g, v) if dir == "out" else ng.inneighbors(g, v)).tolist() == one.tolist()
    with pytest.raises(ng.DimensionMismatch, match=rf"node {n}\b"):
        ng.adjacency_list(g, [0, n], dir)
    with pytest.raises(ng.DimensionMismatch, match=rf"node {n}\b"):
        ng.neighbors(g, n, dir)


def test_adjacency_list_of_a_node_without_edges_and_of_a_star():
    leaves = 5000          # one row longer than any workgroup
    s, t = np.zeros(leaves, np.int64), np.arange(1, leaves + 1)
    g = graph(leaves + 2, s, t)          # node leaves + 1 has no edge
    al = ng.adjacency_list(g, [leaves + 1, 0, 3], "out")
    assert host(al.ptr).tolist() == [0, 0, leaves, leaves] and host(al[1]).tolist() == t.tolist() and al[0].numel() == 0
    assert host(al.eid).tolist() == list(range(leaves))
    check_rows(ng.adjacency_list(g, dir="in"), leaves + 2, s, t, None, "in")
    assert host(ng.inneighbors(g, 17)).tolist() == [0] and ng.outneighbors(g, 17).numel() == 0
    assert host(ng.neighbors(g, 0)).tolist() == t.tolist()


# ---- intersect ------------------------------------------------------------------------------------------------------------------

def check_intersect(got, want, g1):
    ws, wt, weid = want
    gs, gt = got.edge_index(0)
    assert np.array_equal(gs, ws) and np.array_equal(gt, wt) and got.num_nodes == g1.num_nodes and got.num_graphs == g1.num_graphs
    assert got.edge_weight is None and not got.ndata
    if "EID" in got.edata:
        assert got.edata["EID"].dtype == torch.int64 and np.array_equal(host(got.edata["EID"]), weid)
    else:
        assert not got.edata


@pytest.mark.parametrize("n,e", SIZES)
def test_intersect(n, e):
    s, t = edges(n, e)
    g1 = graph(n, s, t)
    own = ng.intersect(g1, g1, return_eid=True)          # g1's distinct pairs in first-appearance order, EID at the first copies
    check_intersect(own, ref_intersect(n, s, t, s, t), g1)
    assert len(own.edata["EID"]) == len(np.unique(s * n + t))
    check_intersect(ng.intersect(g1, graph(n, [], [])), ref_intersect(n, s, t, [], []), g1)
    assert ng.intersect(graph(n, [], []), g1).num_edges == 0
    s3, t3 = random_edges(n, e, seed=5 * n + e + 1)          # a second graph that shares a known half with the first
    half = np.random.default_rng(e).permutation(e)[:e // 2]
    s2, t2 = np.concatenate([s3[:e // 2], s[half]]), np.concatenate([t3[:e // 2], t[half]])
    g2 = graph(n, s2, t2)
    want = ref_intersect(n, s, t, s2, t2)
    assert set(zip(s[half].tolist(), t[half].tolist())) <= set(zip(want[0].tolist(), want[1].tolist()))
    got = ng.intersect(g1, g2, return_eid=True)
    check_intersect(got, want, g1)
    check_intersect(ng.intersect(g1, g2), want, g1)
    again = ng.intersect(g1, g2, return_eid=True)
    assert np.array_equal(again.edge_index(0)[0], got.edge_index(0)[0]) and torch.equal(again.edata["EID"], got.edata["EID"])
    check_intersect(ng.intersect(g2, g1, return_eid=True), ref_intersect(n, s2, t2, s, t), g2)
    with pytest.raises(ng.DimensionMismatch, match="nodes"):
        ng.intersect(g1, graph(n + 1, s, t))


def test_intersect_of_two_radius_graphs_is_the_smaller_one():
    rng = np.random.default_rng(11)
    p = torch.as_tensor(rng.random((2, 400)).astype(np.float32), device=DEV)
    g1, g2 = ng.radius_graph(p, 0.08), ng.radius_graph(p, 0.16)
    assert 0 < g1.num_edges < g2.num_edges
    both = ng.intersect(g1, g2, return_eid=True)
    s1, t1 = g1.edge_index(0)
    assert np.array_equal(both.edge_index(0)[0], s1) and np.array_equal(both.edge_index(0)[1], t1)          # a radius graph has no duplicates
    assert host(both.edata["EID"]).tolist() == list(range(g1.num_edges))
    back = ng.intersect(g2, g1)
    assert set(zip(*[a.tolist() for a in back.edge_index(0)])) == set(zip(s1.tolist(), t1.tolist()))
    assert bool(ng.has_edge(g2, dev64(s1), dev64(t1)).all())


# ---- random_walk_pe: known answers ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 65])
def test_random_walk_on_a_directed_cycle(n):
    K = 2 * n + 3
    g = graph(n, np.arange(n), (np.arange(n) + 1) % n)
    pe = ng.random_walk_pe(g, K)
    assert pe.shape == (K, n) and pe.dtype == torch.float32 and pe.is_cuda
    want = np.array([[1.0 if k % n == 0 else 0.0] * n for k in range(1, K + 1)], np.float32)
    assert np.array_equal(host(pe), want)


def test_random_walk_known_answers():
    pair = ng.random_walk_pe(graph(2, [0, 1], [1, 0]), 6)
    assert host(pair).tolist() == [[0.0, 0.0], [1.0, 1.0]] * 3
    loop = ng.random_walk_pe(graph(1, [0], [0]), 5)
    assert host(loop).tolist() == [[1.0]] * 5
    # node 3 isolated, node 2 a sink (edges enter, none leave), 0 <-> 1
    pe = host(ng.random_walk_pe(graph(4, [0, 1, 0, 1], [1, 0, 2, 2], np.float32([1, 2, 3, 4])), 7))
    assert np.all(np.isfinite(pe)) and np.all(pe[:, 2] == 0) and np.all(pe[:, 3] == 0)
    assert np.all(pe[1::2, :2] > 0) and np.all(pe[0::2, :2] == 0)
    assert ng.random_walk_pe(graph(3, [], []), 2).tolist() == [[0.0] * 3] * 2


# ---- random_walk_pe: against float64 --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def walk_case(n, weighted):
    s, t = random_edges(n, 6 * n, seed=40 + n)
    w = weights(len(s), seed=n) if weighted else None
    return s, t, w, ref_random_walk(n, s, t, w, 8)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("walk_length", [1, 2, 8])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 300])
def test_random_walk_against_float64(n, walk_length, weighted):
    s, t, w, (ref, bound) = walk_case(n, weighted)
    g = graph(n, s, t, w)
    pe = ng.random_walk_pe(g, walk_length, block=64)          # 300 nodes: five blocks, the last one partial
    got = host(pe).astype(np.float64)
    err = np.abs(got - ref[:walk_length])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound[:walk_length] > 0, err / bound[:walk_length], np.where(err > 0, np.inf, 0.0))
    print(f"n {n} K {walk_length} weighted {weighted}: worst |pe - ref| / bound = {ratio.max():.4f}")
    assert np.all(err <= bound[:walk_length]), float(ratio.max())
    assert torch.equal(ng.random_walk_pe(g, walk_length, block=64), pe)


# ---- random_walk_pe: independence -----------------------------------------------------------------------------------------------

def test_random_walk_does_not_depend_on_the_block():
    s, t, w, _ = walk_case(300, True)
    g = graph(300, s, t, w)
    base = ng.random_walk_pe(g, 8, block=64)
    for block in (256, 128, 512, None):
        assert torch.equal(ng.random_walk_pe(g, 8, block=block), base), block
    assert torch.equal(ng.random_walk_pe(ng.adjacency_matrix(g), 8), base)          # the assembled matrix in place of the graph


def test_random_walk_of_a_batch_member_equals_the_solo_run():
    sizes = (65, 1, 300)
    members = []
    for n in sizes:
        s, t = random_edges(n, 5 * n, seed=90 + n)
        members.append(graph(n, s, t, weights(len(s), seed=n + 1)))
    gb = ng.batch(members)
    assert gb.num_graphs == 3 and np.all(np.diff(gb.graph_indicator) >= 0)
    K = 6
    solo = [ng.random_walk_pe(m, K, block=64) for m in members]
    want = torch.cat(solo, dim=1)
    for block in (64, 256):
        assert torch.equal(ng.random_walk_pe(gb, K, block=block), want), block
    # the same batch with the graphs interleaved (every graph's nodes keep their order, so every row keeps its column order): the
    # indicator is no longer non-decreasing and every launch covers all rows
    gi = np.random.default_rng(3).permutation(gb.graph_indicator)
    assert np.any(np.diff(gi) < 0)
    new_of = np.empty(gb.num_nodes, np.int64)          # new position of every old node
    for k in range(3):
        new_of[gb.graph_indicator == k] = np.flatnonzero(gi == k)
    s, t = gb.edge_index(0)
    shuffled = graph(gb.num_nodes, new_of[s], new_of[t], np.asarray(gb.edge_weight, np.float32), graph_indicator=gi, num_graphs=3)
    for block in (64, 256):
        pe = ng.random_walk_pe(shuffled, K, block=block)
        assert torch.equal(pe[:, torch.as_tensor(new_of, device=DEV)], want), block


# ---- random_walk_pe: arguments ----------------------------------------------------------------------------------------------------

def test_random_walk_arguments():
    s, t, w, _ = walk_case(65, True)
    g = graph(65, s, t, w)
    with pytest.raises(ng.ArgumentError, match="walk_length"):
        ng.random_walk_pe(g, 0)
    for block in (63, 100, 0):
        with pytest.raises(ng.ArgumentError, match="multiple of 64"):
            ng.random_walk_pe(g, 2, block=block)
    a = ng.adjacency_matrix(g)
    lib = _lib.load()
    need = lib.ngpde_csr_random_walk_pe_workspace_bytes(65, 64)
    pe = torch.full((2, 65), -1.0, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = lib.ngpde_csr_random_walk_pe(65, a.nnz, _lib.ptr(a.row_ptr), _lib.ptr(a.cols), _lib.ptr(a.values), 1, None, 2, 64, _lib.ptr(pe), _lib.ptr(ws),
                                      need - 1, _lib.current_stream())
    assert st == _lib.ERR_WORKSPACE and b"needed" in lib.ngpde_last_error()
    torch.cuda.synchronize()
    assert bool((pe == -1.0).all())          # refused before any launch
    st = lib.ngpde_csr_random_walk_pe(65, a.nnz, _lib.ptr(a.row_ptr), _lib.ptr(a.cols), _lib.ptr(a.values), 1, None, 2, 64, _lib.ptr(pe), _lib.ptr(ws),
                                      need, _lib.current_stream())
    assert st == 0 and torch.equal(pe, ng.random_walk_pe(g, 2, block=64))


# ---- HIP-graph capture ----------------------------------------------------------------------------------------------------------

def test_capture_replays_the_eager_result():
    s, t, w, _ = walk_case(300, True)
    g = graph(300, s, t, w)
    a = ng.adjacency_matrix(g)
    rng = np.random.default_rng(5)
    qs, qt = dev64(np.concatenate([s[:200], rng.integers(0, 300, 200)])), dev64(np.concatenate([t[:200], rng.integers(0, 300, 200)]))

    def step():
        return ng.has_edge(g, qs, qt), ng.has_edge(g, qs, qt, return_eid=True), ng.random_walk_pe(a, 4, block=64), ng.random_walk_pe(a, 3)

    eager = [x.clone() for x in step()]          # (the key plan is sorted here, outside the capture)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    gc_was = gc.isenabled()
    gc.disable()                                    # (a finaliser that frees device memory must not run inside the capture)
    try:
        with torch.cuda.graph(gr):
            outs = step()
    finally:
        if gc_was:
            gc.enable()
    for _ in range(2):
        for x in outs:
            x.zero_()
        gr.replay()
        torch.cuda.synchronize()
        for x, y in zip(outs, eager):
            assert torch.equal(x, y)
